// rp_kernels.h -- launchers of the gfx950 kernels (rp_mfcc / rp_dtw / rp_scan / rp_resample / rp_frontend / rp_mlp / rp_average .hip) used by the
// host-side mirror (rp_detector.cpp) and the C ABI (rp_capi.cpp, rp_stream_batch.cpp).
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rp {

constexpr int kFrame = 480;   // src/constants.rs:2 @16 kHz
constexpr int kShift = 160;   // src/constants.rs:8
constexpr int kBins = 240;    // src/mfcc/extractor.rs:28

// Device-resident constant tables of the MFCC pipeline for one mfcc_size K.
// mfcc_size 5 / 16 (K1 = 6 / 17 filters): can filter f be non-zero on a bin of the 16-bin group k2 (bins l + 16*k2,
// l = 0..15), or -- mirror -- on a bin 240 - (l + 16*k2)?  Triangle f is non-zero on bins (c[f], c[f+2]) exclusive;
// the centres are what new_mel_filter_bank (src/mfcc/extractor.rs:164-198) yields for these sizes (checked against
// the table on upload, Ctx::tables_for).
template <int K1T> struct MelCentres;
template <> struct MelCentres<6> { static constexpr int c[8] = {0, 9, 22, 41, 68, 106, 161, 240}; };
template <> struct MelCentres<14> { static constexpr int c[16] = {0, 4, 8, 14, 20, 28, 37, 47, 60, 74, 92, 112, 137, 166, 200, 240}; };
template <> struct MelCentres<17> {
    static constexpr int c[19] = {0, 3, 7, 11, 16, 21, 28, 35, 43, 53, 64, 77, 92, 109, 128, 150, 176, 206, 240};
};
template <int K1T> __host__ __device__ constexpr bool mel_touches(int f, int k2, bool mirror) {
    if (f < 0 || f >= K1T) return false;
    const int lo = MelCentres<K1T>::c[f] + 1, hi = MelCentres<K1T>::c[f + 2] - 1;  // non-zero bins lo..hi
    const int g_lo = mirror ? 240 - (16 * k2 + 15) : 16 * k2;                        // bins the group covers
    const int g_hi = mirror ? 240 - 16 * k2 : 16 * k2 + 15;
    return g_hi >= lo && g_lo <= hi;
}

// The sparse mel tables of the mfcc_size 5 / 16 kernels: per lane l (= bin residue mod 16) the weights of exactly the
// (filter, 16-bin group, direct / mirror) triples mel_touches<K1T> admits, in the order the kernel accumulates them
// (filter ascending, group ascending, direct before mirror) -- one contiguous row of kMelRowPitch<K1T> floats per lane,
// read with 16-byte LDS loads (a pitch of 36 / 44 floats keeps the 16 lanes of a frame on distinct banks).
template <int K1T> __host__ __device__ constexpr int mel_index(int f, int k2, bool mirror) {
    int n = 0;
    for (int ff = 0; ff < K1T; ++ff)
        for (int kk = 0; kk < 8; ++kk) {
            if (ff == f && kk == k2 && !mirror) return n;
            if (mel_touches<K1T>(ff, kk, false)) ++n;
            if (ff == f && kk == k2 && mirror) return n;
            if (mel_touches<K1T>(ff, kk, true)) ++n;
        }
    return n;  // f == K1T: the number of entries
}
template <int K1T> constexpr int kMelEntries = mel_index<K1T>(K1T, 0, false);
template <int K1T> constexpr int kMelRowPitch = ((kMelEntries<K1T> + 3) / 4) * 4 + (((kMelEntries<K1T> + 3) / 4) % 2 == 0 ? 4 : 0);  // 16-byte units: odd count
static_assert(kMelEntries<6> == 31 && kMelRowPitch<6> == 36 && kMelEntries<17> == 41 && kMelRowPitch<17> == 44, "mel table shape");

struct MfccTablesDev {
    int K1 = 0;               // K+1 filters / cepstral coefficients
    bool mel_sparse = false;  // K1 is 6 or 17 and the mel bank is non-zero only where mel_touches<K1> says (checked on upload)
    float *hamming = nullptr; // [480]
    float2 *tw240 = nullptr;  // [240] exp(-2*pi*i*k/240)
    float2 *tw480 = nullptr;  // [240] exp(-2*pi*i*k/480)
    float *fb = nullptr;      // [K1][240]
    float *melw = nullptr;    // mel_sparse: [16][kMelRowPitch<K1>] compact per-lane weights (mel_index order)
    float *dct = nullptr;     // [K1][K1] cos table, row k col n
};

// Templates of one length that one wave scores together (register kernel).
constexpr int kChunkMax = 8;
struct DtwChunk {
    int len;              // frames of every template in the chunk
    int count;            // real templates, 1..tc
    int tc;               // register tile the kernel is instantiated for: 2, 4 or 8
    int rows_off;         // float offset of the chunk's rows in TemplatesDev::dup
    int tid[kChunkMax];   // output column of each template; T means the averaged template
    int aimg_off;         // chunks of 3..8 templates at mfcc_size 5: offset (16-byte units) of the chunk's A image in TemplatesDev::aimg
    int aimg3_off;        // ... of its three-part bf16 image in TemplatesDev::aimg3 (kDtwMfma3RowBytes per row)
};

// dtw_mfma_kernel (rp_dtw_mfma.hip): A image = per template row [k half 2][template 8] x 8 f16 (the negated unit row, split in two f16
// parts, in the slot order of the MFMA's B operand) for len + 16 rows (the tail rows are zero); per wave two stream segments of frames.
constexpr int kDtwMfmaRowBytes = 256;
// The f32-grade form (rp_ctx arithmetic RP_ARITH_F32_MATRIX, the default): the negated unit row as THREE bf16 parts a0 + a1 + a2 (exact: 3 x 8
// significant bits = an f32's 24), two k-steps of 16 slots per row = [k-step 2][k half 2][template 8] x 8 bf16.
constexpr int kDtwMfma3RowBytes = 512;
__host__ __device__ inline int dtw_mfma_stage_floats(int max_len) { return ((32 + 2 * (max_len + 3)) * 5 + 3) & ~3; }
// dtw_mfma_wide_kernel (mfcc_size 13 / 16): components per lane half and k-steps of 16 f16 slots (rp_dtw_mfma_wide.hip)
__host__ __device__ constexpr int dtw_mfma_wide_chm(int K) { return (K + 1) / 2; }
__host__ __device__ constexpr int dtw_mfma_wide_ksteps(int K) {
    return (3 * (dtw_mfma_wide_chm(K) / 2) + (dtw_mfma_wide_chm(K) % 2 ? 2 : 0) + 3) / 4;
}
// bytes from one template row of the wide A image to the next: the k-steps' 256-byte blocks + 128 -- a ds_read_b128 takes 16 lanes at a
// time = two row slots x 128 bytes; a pitch that is a multiple of 256 bytes put both on the same 32 banks (SQ_LDS_BANK_CONFLICT = half of
// the kernel's LDS cycles, profiles/r05_wide_pmc.txt)
__host__ __device__ constexpr int dtw_mfma_wide_row_bytes(int K) { return dtw_mfma_wide_ksteps(K) * 256 + 128; }
// dtw_mfma_wide3_kernel (rp_dtw_mfma_wide3.hip; mfcc_size 13 / 16 in the three-part bf16 arithmetic): FOUR template slots per wave, six k-steps
// of 16 slots; A image = per template row [k-step 6][k half 2][template 4] x 8 bf16 = 768 bytes + 64 (the four row slots a ds_read_b128 serves
// fall on different banks)
constexpr int kDtwWide3KSteps = 6;
constexpr int kDtwWide3RowBytes = kDtwWide3KSteps * 128 + 64;
// The window side's operand of a lane half is ONE run of twelve registers read in overlapping four-register pieces at offsets 0, 2, 4, 4, 6, 8
// (rp_dtw_mfma_wide3.hip, w3_run_piece):
//   mfcc_size 16 (four component pairs a..d):          [P2a P2b P1a P1b P0a P0b P0c P0d P1c P1d P2c P2d]
//   mfcc_size 13 (three pairs a..c + one component s): [P2a P2b P1a P1b P0a P0b P0c S01 P1c S2C P2c  0 ]
// with Pk of a pair = (xk of its first component, xk of its second), S01 = (x0s, x1s), S2C = (x2s, the 1.0 of 1 - a.x in half 1).  Slot i of
// k-step ks of the A image holds the template parts that complete the products: W3Slot{component, part} for the slot's two bf16 (component
// within the lane half; -1: zero; -2: the constant's 1.0, half 1 only).  S01 is read three times -- against (a0s, a0s), (a1s, a1s), (a2s, 0) --
// so the odd component needs no register of its own per product; registers read more often than they have products meet zeros.
struct W3Slot { int c0, p0, c1, p1; };
__host__ __device__ constexpr W3Slot dtw_mfma_wide3_slot(int K, int ks, int i) {
    constexpr int pair16[6][4] = {{0, 1, 0, 1}, {0, 1, 0, 1}, {0, 1, 2, 3}, {0, 1, 2, 3}, {2, 3, 2, 3}, {2, 3, 2, 3}};
    constexpr int part16[6][4] = {{0, 0, 0, 0}, {1, 1, 0, 0}, {1, 1, 0, 0}, {2, 2, 1, 1}, {2, 2, 0, 0}, {1, 1, 0, 0}};
    constexpr W3Slot s13[6][4] = {
        {{0, 0, 1, 0}, {2, 0, 3, 0}, {0, 0, 1, 0}, {2, 0, 3, 0}},      // P2a P2b P1a P1b  x a0
        {{0, 1, 1, 1}, {2, 1, 3, 1}, {0, 0, 1, 0}, {2, 0, 3, 0}},      // P1a P1b x a1, P0a P0b x a0
        {{0, 1, 1, 1}, {2, 1, 3, 1}, {4, 0, 5, 0}, {6, 0, 6, 0}},      // P0a P0b x a1, P0c x a0, S01 x (a0s, a0s)
        {{0, 2, 1, 2}, {2, 2, 3, 2}, {4, 1, 5, 1}, {6, 1, 6, 1}},      // P0a P0b x a2, P0c x a1, S01 x (a1s, a1s)
        {{4, 2, 5, 2}, {6, 2, -1, 0}, {4, 0, 5, 0}, {6, 0, -2, 0}},    // P0c x a2, S01 x (a2s, 0), P1c x a0, S2C x (a0s, 1.0)
        {{4, 1, 5, 1}, {-1, 0, -1, 0}, {4, 0, 5, 0}, {-1, 0, -1, 0}}}; // P1c x a1, S2C x 0, P2c x a0, 0 x 0
    return K == 16 ? W3Slot{2 * pair16[ks][i], part16[ks][i], 2 * pair16[ks][i] + 1, part16[ks][i]} : s13[ks][i];
}
// Tiles a wave of the matrix-core DTW kernels takes by its own index before it turns to the chunk's atomic counter: every whole round
// of a launch of at most three rounds (live-stream calls, BASELINE config C2 -- the waves start together and would ask for their
// tickets together; the counter then hands out what is left), the first round of longer launches (the waves drift apart by themselves
// and the counter evens out what the CUs finish unevenly) and of lists whose length only the device knows.
inline unsigned mfma_static_rounds(size_t total_tiles, size_t chunk_waves, bool list) {
    const size_t r = chunk_waves ? total_tiles / chunk_waves : 0;
    if (const char *e = std::getenv("RP_MFMA_STATIC_ROUNDS")) return (unsigned)std::atoi(e);  // A/B runs: 0 = every tile from the counter
    return (list || r > 3 || r < 1) ? 1u : (unsigned)r;
}
// compute units of the current device (cached per device)
int device_cu_count();
// Grid of the matrix-core DTW kernels: the CUs split over the n_chunks chunks (at least one workgroup each), a chunk's workgroups no more
// than its rounds of `waves` tiles; and the rounds a wave takes by index.  The tile counter words (DtwWork::sched) are zero between
// launches; the kernels' side of that protocol is dtw_next_tile / dtw_release_tiles (rp_device.h).
inline hipError_t mfma_grid(size_t total_tiles, int n_chunks, int waves, bool list, unsigned &blocks, unsigned &static_rounds) {
    size_t groups = (size_t)device_cu_count() / (size_t)n_chunks;
    if (groups < 1) groups = 1;
    const size_t need = (total_tiles + waves - 1) / waves;
    if (groups > need) groups = need;
    if (groups * (size_t)n_chunks > 0x7fffffffULL) return hipErrorInvalidValue;
    blocks = (unsigned)(groups * (size_t)n_chunks);
    static_rounds = mfma_static_rounds(total_tiles, groups * (size_t)waves, list);
    return hipSuccess;
}
inline size_t dtw_mfma_lds_bytes(int max_len, int waves, int row_bytes = kDtwMfmaRowBytes) {
    return (size_t)(max_len + 16) * (size_t)row_bytes + (size_t)waves * (size_t)dtw_mfma_stage_floats(max_len) * sizeof(float);
}

// The arithmetic a context asks of the DTW launchers (rp_ctx_new flags / rp_ctx_set_arithmetic, include/rustpotter_hip.h RP_ARITH_*): read per
// call through TemplatesDev::arith, so that one template set serves every mode.
//   kArithF32Matrix (default): matrix-core kernels only in their f32-grade form -- operands as three bf16 parts (exact), six of the nine partial
//     products of a multiplication (what is dropped is below 2^-22 of it, 2^-25.7 rms: an f32 multiply itself rounds by up to 2^-24) -- and the
//     f32 vector kernels wherever no such form exists;
//   kArithStrictF32: the f32 vector ("register") kernels only, every product an f32 FMA;
//   kArithFastSplit: the two-part f16 forms of rounds 3-5 (22-bit operands, one partial product dropped): dtw_mfma_kernel, dtw_mfma_group_kernel,
//     dtw_mfma_wide_kernel; `ragged` additionally admits dtw_ragged_kernel (same two-part arithmetic on per-stream offsets).
enum { kArithF32Matrix = 0, kArithStrictF32 = 1, kArithFastSplit = 2 };
struct DtwArith {
    int mode = kArithF32Matrix;
    int ragged = 0;
};

// Device-resident template set of one wakeword reference.
struct TemplatesDev {
    const DtwArith *arith = nullptr;   // the owning context's setting (host memory; null = defaults)
    int arith_mode() const { return arith ? arith->mode : (int)kArithF32Matrix; }
    bool arith_ragged() const { return arith && arith->mode == kArithFastSplit && arith->ragged; }
    int T = 0;        // sample templates
    int K = 0;
    int Lpad = 0;     // row pitch (frames) of `unit`
    int has_avg = 0;  // template index T is the averaged template
    int max_len = 0;  // max over sample templates
    int max_diff = 0; // max(0, longest template incl. avg - max_len): >0 forces the generic kernel
    int *lens = nullptr;   // [T+has_avg]
    float *unit = nullptr; // [T+has_avg][Lpad][K] rows scaled to unit L2 norm (zero rows stay zero)
    // register-kernel layout: chunks sorted by class (see class_first); dup holds per chunk [len][tc/2][K][2]: the coefficients of two templates
    // interleaved, so that one scalar 8-byte load feeds both halves of a packed f32 FMA.
    DtwChunk *chunks = nullptr;
    float *dup = nullptr;
    // chunk classes: 0 = two templates (tc 2), 1 = three or four (tc 4), 2 = five to eight (tc 8), 3 = ONE template (scored two
    // windows per lane by dtw_band2_kernel; the averaged template is the LAST chunk of class 3)
    int class_first[4] = {0, 0, 0, 0};
    int class_count[4] = {0, 0, 0, 0};
    // every class-2 chunk once more as two tc-4 halves (only when each of them holds 7 or 8 templates): a small batch whose
    // tc-8 waves would fill the chip 2.x times is scored by twice as many tc-4 waves, three resident per SIMD instead of two
    int split_first = 0, split_count = 0;
    // dtw_mfma_kernel: A images of the class-1 and class-2 chunks (mfcc_size 5 only), and the shortest template among them
    void *aimg = nullptr;
    void *aimg3 = nullptr;  // the same chunks' three-part bf16 images (kDtwMfma3RowBytes per row, DtwChunk::aimg3_off)
    int mfma_min_len = 0;   // shortest template among the class-2 chunks (8 template slots; needs >= 12 frames)
    int mfma_min_len4 = 0;  // ... among the class-1 chunks (4 template slots; needs >= 16 frames)
    // mfcc_size 13 / 16: the sample templates once more as chunks of up to 8 same-length templates for dtw_mfma_wide_kernel (only when
    // every length occurs at least three times: the matrix kernel always pays for eight template slots)
    int wide8_first = 0, wide8_count = 0;
    // ... and as chunks of up to 4 for dtw_mfma_wide3_kernel (three-part bf16 images in aimg3, DtwChunk::aimg3_off)
    int wide4_first = 0, wide4_count = 0, wide4_min_len = 0;
    int n_chunks_total = 0;   // entries of `chunks` that index tile counters (all but the ragged chunks at its end; the counters live in the CALL's workspace, DtwWork::sched)
    // The reference forms the cosine as dot_ab / sqrt(dot_a * dot_b) in f32 (comparator.rs:28-48): the PRODUCT of the squared norms
    // can underflow (-> "magnitude == 0" -> similarity 0) or overflow where neither factor does.  The kernels above are scale
    // invariant (unit-length rows and frames), so they only agree with it while both squared norms stay in a range where the product
    // is a normal f32: kDtwNormLo..kDtwNormHiRow for template rows (checked here, on upload), ..kDtwNormHiFrame for window frames
    // (checked by every kernel, per frame).  `raw` = the rows as given, for the reference-shaped cell of dtw_ref_kernel; ref_only:
    // some row is outside the range -- every window of this set is scored by dtw_ref_kernel.
    float *raw = nullptr;     // [T+has_avg][Lpad][K]
    int ref_only = 0;
    // dtw_mfma_group_kernel (rp_dtw_mfma_group.hip): runs of 4 consecutive class-2 chunks of one template length, grp_first[] (device) the
    // first chunk of each; rest_*: the class-2 chunks outside every group, as runs for dtw_mfma_kernel
    int *grp_first = nullptr;
    int grp_count = 0, grp4_max_len = 0;
    int rest_runs = 0, rest_first[8] = {0, 0, 0, 0, 0, 0, 0, 0}, rest_count[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // dtw_ragged_kernel (rp_dtw_ragged.hip, mfcc_size 5): the sample templates the equal-length matrix kernel does not take (lengths that
    // occur once or twice) as chunks of up to 8 templates of ANY lengths, shortest first; rimg = per template its A image, 32 bytes per
    // row ([k half 2] x 8 f16: the negated unit row split in two f16 parts) + 16 zero rows, rag_off[t] its offset in 16-byte units
    int rag_first = 0, rag_count = 0;
    int rag_min_len = 0;      // shortest template among them (needs >= 16 frames)
    int rag_a_cap = 0;        // largest chunk's images in bytes
    int rag_rows_cap = 0;     // ... unit rows in floats (multiple of 4)
    void *rimg = nullptr;
    int *rag_off = nullptr;   // [T]
};
// squared-norm range in which the scale-invariant cell equals the reference's: 2^-60 <= |row|^2 <= 2^60, 2^-60 <= |frame|^2 <= 2^30
// (products stay within 2^-120 .. 2^90; a frame is tested with ONE v_max3_f32 of its squared norm and its reciprocal square root
// against 2^30).  Zero rows / frames are exact in both forms (similarity 0).
constexpr float kDtwNormLo = 8.673617379884035e-19f, kDtwNormHiRow = 1.152921504606847e18f, kDtwFixLimit = 1073741824.f;

// Per-CALL device workspace of the DTW launchers (owned by the context, Ctx::dtw_work): the tile counters of the matrix-core kernels
// ({next tile, workgroups done} per chunk, zero between launches: the last workgroup of a launch puts them back) and the list of
// (window, chunk) pairs whose frames left the range above (fix[0] = entries appended, fix[1] = workgroups of dtw_ref_kernel done,
// entries from fix[2] on as 64-bit words row << 24 | spec).  Calls on one context are serialised (one stream), so the words are
// never shared by two launches.
constexpr int kDtwSchedChunks = 2048;       // chunks of one template set the counters cover
constexpr uint32_t kDtwFixCap = 1u << 18;   // listed (window, chunk) pairs; beyond: every window of the call is rescored
constexpr uint32_t kFixSpecTemplate = 1u << 22, kFixSpecAll = 1u << 23, kFixSpecMask = (1u << 24) - 1;
struct DtwWork {
    uint32_t *sched = nullptr;   // [2 * kDtwSchedChunks]
    uint32_t *fix = nullptr;     // [2 + 2 * kDtwFixCap + 2]: the last two words count the pairs rescored since the context was made
    uint32_t *ran = nullptr;     // HOST word (may be null): the launchers OR in the kernel families they launched (kDtwRan*, rp_ctx_dtw_kernels)
    // dtw_ragged_kernel's per-call device blocks (Ctx::dtw_work_for; null: that kernel is not taken): rag_prep [rag_streams][8] floats
    // (offset and scale of every stream), rag_list [1 + rag_rows] words (the windows to score again with the register kernels; rows x ragged chunks)
    float *rag_prep = nullptr;
    uint32_t *rag_list = nullptr;
    size_t rag_streams = 0, rag_rows = 0;
};
// == RP_DTW_KERNEL_* (include/rustpotter_hip.h)
enum : uint32_t { kDtwRanMfma = 1u, kDtwRanMfmaWide = 2u, kDtwRanRagged = 4u, kDtwRanRegister = 8u, kDtwRanGeneric = 16u, kDtwRanSingle = 32u, kDtwRanRefAll = 64u, kDtwRanMfmaGroup = 128u,
                  // the product arithmetic of the matrix-core launches: three bf16 parts (f32-grade) / two f16 parts (22-bit)
                  kDtwRanBf16x3 = 256u, kDtwRanF16x2 = 512u,
                  // waves per workgroup of the dtw_mfma_kernel launches (two / three per SIMD)
                  kDtwRanWaves8 = 1024u, kDtwRanWaves12 = 2048u,
                  // dtw_bank_kernel (rp_dtw_bank.hip): per-stream wakewords from a bank
                  kDtwRanBank = 4096u,
                  // dtw_bank_stream_kernel (rp_dtw_bank.hip): the same for the new windows of a live-stream batch
                  kDtwRanBankStream = 8192u,
                  // dtw_set_kernel / dtw_set_stream_kernel (rp_dtw_set.hip): a set of wakewords of a bank per stream
                  kDtwRanBankSets = 16384u, kDtwRanBankSetsStream = 32768u,
                  // dtw_mixed_stream_kernel (rp_dtw_set.hip): the reference slots of a live-stream batch over mixed sets
                  kDtwRanMixedSetsStream = 65536u };
inline void dtw_mark(const DtwWork &wk, uint32_t bit) { if (wk.ran) *wk.ran |= bit; }
__host__ __device__ inline unsigned long long *dtw_fix_stats(uint32_t *fix) { return reinterpret_cast<unsigned long long *>(fix + 2 + 2 * (size_t)kDtwFixCap); }
// (dtw_fix_append, the kernels' side of the list: rp_device.h)

// ScoreMode::Max folded into the matrix-core DTW kernel when ONE chunk holds every sample template of the reference and no averaged
// template is scored in the call (BASELINE C2 / C3, a live-stream call with same-length templates): the lane pair of a window holds all
// its scores, so the kernel also writes agg[row] = max_t score and raises the stream's `hot` flag like agg_store (rp_dtw.hip) -- the
// aggregate pass (a launch, and a second read of every score) is skipped.  launch_dtw sets `done` when it took that route.
struct DtwFusedAgg {
    float *agg = nullptr;
    uint32_t *hot = nullptr;   // one flag per stream, zero before the launch (Ctx::hot_flags: the scan leaves them so); may be null
    float threshold = 0.f;
    bool done = false;
};

// The gate / abandon mode of ONE launch: the averaged-template gate's hand-over to the template kernels (launch_dtw_gated).  count ==
// nullptr: no gate, every window is scored.  list != nullptr: LIST mode -- the lanes take the listed rows (windows that passed) and read
// their frames from global memory; the launch does nothing when the list is dense (*count >= dense_min).  list == nullptr with a count:
// DENSE mode -- the ordinary LDS-staged launch over every window, which does nothing unless the list is dense.  (Nearly everything
// passing is the common case at the reference's default threshold; scoring all rows through the staged kernel is then ~6 % cheaper than
// gathering them one by one.  Both launches are always issued; one of them exits on a scalar compare.)
// The register kernels of rp_dtw.hip take it by value: the fields keep their offsets.
struct GateList {
    const uint32_t *list = nullptr, *count = nullptr;
    uint32_t dense_min = 0;
    // entries the list may hold per row of the call (1: the gate lists a row once; dtw_ragged_kernel's list holds a window once per ragged
    // chunk that could not resolve it): the list-mode grids cover S x n_win x list_mult entries
    uint32_t list_mult = 1;
    // Early abandon (detect-only calls in ScoreMode::Max): a DTW whose cheapest band cell already costs more than
    // abandon_nc * (m + n) cannot end with a score above the detection threshold (cell costs are >= 0 and every warping
    // path crosses every row), so a wave whose 64 windows x templates are ALL past that bound stops and reports score 0 for
    // them.  Windows that can still fire are never touched: their wave runs to the end, with every template exact.
    // +inf: off (the per-window score arrays are part of the call's result).  See dtw_abandon_nc().
    float abandon_nc = __builtin_inff();
    const DtwFusedAgg *fuse = nullptr;  // ScoreMode::Max folded into the matrix-core kernel; set by launch_dtw_fast only
    // DtwWork::fix for the register kernels: windows with a frame whose squared norm leaves kDtwNormLo..kDtwFixLimit are listed for
    // dtw_ref_kernel (the reference's sqrt(dot_a * dot_b) is not scale invariant there, comparator.rs:42-47); their launchers set it
    uint32_t *fix = nullptr;
};

// What is fixed for one scoring call: dtw_score builds it once and every launcher below it takes it, plus what varies per launch (chunk
// range, template slots, from_global, the GateList).  mfcc rows have frame_pitch frames per stream, scores / avg rows out_win_pitch windows.
struct DtwCall {
    hipStream_t st = nullptr;
    DtwWork wk;
    const TemplatesDev *t = nullptr;
    const float *mfcc = nullptr;
    size_t S = 0, frame_pitch = 0, first_win = 0, n_win = 0, out_win_pitch = 0;
    int band = 0;
    float score_ref = 0.f;
    float *scores = nullptr, *avg = nullptr;
    bool padded_rows = false;   // the frame array ends with slack (DtwScore::padded_rows)
};

// The matrix-core DTW kernel (rp_dtw_mfma.hip) for the chunks of class 2 (5..8 templates; slots = 8, band 3..5) and class 1 (3..4
// templates; slots = 4, band 5) at mfcc_size 5.  from_global: lanes read their frames from global memory (live-stream batches, LIST mode
// of the averaged-template gate) instead of an LDS stage (needs n_win >= 32).
// score_ref: the relative error of a score is (1 - score) x d(cost / (m + n)) / score_ref; the split products keep it within the parity
// gate (1e-5) down to kDtwMfmaMinScoreRef (tools/probe_score_ref.py, tests/test_gpu_round4.py); below, the f32 register kernels score
constexpr float kDtwMfmaMinScoreRef = 0.05f;
bool dtw_mfma_supported(const TemplatesDev &t, int band, size_t n_win, bool from_global, int slots, float score_ref);
hipError_t launch_dtw_mfma(const DtwCall &c, int slots, int chunk_base, int n_chunks, bool from_global, const GateList &gate);
// mfcc_size 13 / 16 at band 5: frames always from global memory (the caller's rows end with slack: DtwScore::padded_rows)
bool dtw_mfma_wide_supported(const TemplatesDev &t, int band, float score_ref);
hipError_t launch_dtw_mfma_wide(const DtwCall &c, const GateList &gate);
// the same shapes in the default arithmetic (three bf16 parts per operand, no score_ref floor): chunks of up to four templates
bool dtw_mfma_wide3_supported(const TemplatesDev &t, int band);
hipError_t launch_dtw_mfma_wide3(const DtwCall &c, const GateList &gate);
size_t dtw_mfma_group_lds_bytes(int L, int sh);
bool dtw_mfma_group_supported(const TemplatesDev &t, int band, size_t n_win, size_t S, float score_ref);
hipError_t launch_dtw_mfma_group(const DtwCall &c);

// The matrix-core DTW kernel for templates of unequal length (rp_dtw_ragged.hip): the ragged chunks of `t` over every window of the call
// (LDS-staged tiles of 512 windows: needs n_win >= 64; live-stream batches and the gate's list keep the register kernels).
constexpr int kDtwRaggedWaves = 8;    // waves per workgroup = 512 windows per tile
constexpr int kDtwRaggedSegs = 16;    // stream segments a tile may span
// the cell error is 2^-22 x |x_f - o| / |x_f - mu| (a few times dtw_mfma_kernel's): floor of score_ref for the 1e-5 parity gate
constexpr float kDtwRaggedMinScoreRef = 0.1f;
bool dtw_ragged_supported(const TemplatesDev &t, int band, size_t n_win, float score_ref);
size_t dtw_ragged_lds_bytes(const TemplatesDev &t, size_t n_win, int *frames_cap);
// list_rows: windows the kernel cannot score within the parity gate go to wk.rag_list (the caller runs the register kernels' list mode on it);
// else to wk.fix (dtw_ref_kernel)
hipError_t launch_dtw_ragged(const DtwCall &c, float abandon_nc, bool list_rows);

// ---- wakeword bank (rp_dtw_bank.hip, rp_bank.cpp): W wakeword references resident on the device, scored per stream through an index.
// Every template of the bank (the sample templates of wakeword 0, of wakeword 1, ..., then the averaged templates) is one entry of tlen /
// trow; its rows lie at unit / raw + trow * K (unit: scaled to unit length as in TemplatesDev; raw: as given, for the reference-shaped cell).
constexpr int kBankMaxTemplates = 32;   // sample templates per wakeword: the LDS block of the percentile modes is [32][64] floats
struct BankWakeword {
    int first;        // entry of its first sample template
    int count;        // sample templates, 1..kBankMaxTemplates
    int max_len;      // longest sample template = the window length (get_mfcc_frame_size, wakeword_comp.rs:69-75)
    int avg;          // entry of its averaged template, -1: none
    int ref_only;     // a row outside kDtwNormLo..kDtwNormHiRow: every window of this wakeword takes the reference-shaped cell
    float threshold, avg_threshold;   // the wakeword's own Option<f32>: NaN = the value of the call's config
    int window_chk;   // the norm-range test reads the window's own frames only, as dtw_generic_kernel: !dtw_register_staged(K, max_len)
};
struct BankDev {
    int W = 0, K = 0;
    int max_len = 0, min_len = 0;     // longest / shortest window length over the wakewords (0 / 0 for an empty bank)
    BankWakeword *ww = nullptr;       // [W]
    int *tlen = nullptr;              // [entries]
    long long *trow = nullptr;        // [entries]
    float *unit = nullptr, *raw = nullptr;
};
// One scoring call of a bank: stream s scores the windows of its own wakeword stream_wakeword[s] (outside [0, W): none).  Outputs are rows of
// win_pitch floats per stream: the windows the stream has, zeros behind them.
struct BankScore {
    const float *mfcc = nullptr;      // [S][n_frames][K]
    size_t S = 0, n_frames = 0, win_pitch = 0;
    const int32_t *stream_wakeword = nullptr;
    int band = 0, score_mode = 0;
    float score_ref = 0.f;
    int avg_mode = 0;                 // the averaged template is scored: 0 never, 1 where a wakeword has one, 2 ... and its effective avg_threshold != 0
    int gate = 0;                     // detect-only: a wave none of whose windows passes avg_threshold skips the sample templates; rejected windows get aggregate 0
    float threshold = 0.f, avg_threshold = 0.f;   // the config's values (a wakeword's own override them)
    float *agg = nullptr, *avg = nullptr;         // [S][win_pitch]; avg may be null
    uint32_t *hot = nullptr;          // [S] (optional), zero before the call: raised for streams with a window that can fire
    uint32_t *fix = nullptr;          // DtwWork::fix: its statistics words count the pairs scored with the reference-shaped cell
};
// Do the register kernels take a window of max_len frames?  They stage two tiles of 64 windows + two window lengths of frames in the CU's
// 160 KB (windows up to 4 024 / 1 503 / 1 132 frames at mfcc_size 5 / 13 / 16); rp_templates with a longer window are scored by
// dtw_generic_kernel in every call shape (dtw_route), which loads no frame behind a window's end -- so its norm-range test never sees one, and a bank wakeword
// of that length must not either if it is to give the same bits (BankWakeword::window_chk).
inline bool dtw_register_staged(int K, int max_len) {
    return (size_t)(2 * 64 + 2 * (max_len + 8)) * (size_t)(K | 1) * sizeof(float) <= 160 * 1024;
}
// LDS of one wave: the staged frames of a tile for the bank's longest window, the percentile block, the band of the reference-shaped cell
inline size_t dtw_bank_lds_bytes(int K, int max_len) {
    return ((size_t)(64 + max_len + 6) * (size_t)(K | 1) + (size_t)kBankMaxTemplates * 64 + 13 * 64) * sizeof(float);
}
// built for dtw_register_tile(K, band) > 0 (hipErrorNotSupported otherwise; band 0 is the caller's: all-zero scores)
hipError_t launch_dtw_bank(hipStream_t st, const BankDev &b, const BankScore &q);
// One call of a live-stream batch over a bank (rp_stream_batch_new_bank): stream s scores, against its own wakeword, the n_new windows that
// end at its new frames first_new .. first_new + n_new - 1 of its MFCC row (frame_pitch frames a stream, as the GX forms of rp_dtw.hip; the
// window of max_len(s) frames starts max_len(s) - 1 frames before its last one, so first_new >= the bank's max_len - 1).  The band reads up
// to `band` frames behind a window's end: the rows end with that slack.  agg / avg [S][n_new]; a stream without a wakeword gets zero rows.
// The averaged template is scored where a wakeword has one and its effective avg_threshold != 0 (BankScore::avg_mode 2).
struct BankStreamScore {
    const float *mfcc = nullptr;      // [S][frame_pitch][K]
    size_t S = 0, frame_pitch = 0, first_new = 0, n_new = 0;
    const int32_t *stream_wakeword = nullptr;
    int band = 0, score_mode = 0;
    float score_ref = 0.f;
    int gate = 0;                     // detect-only: a window below its avg_threshold is not compared with the sample templates (aggregate 0)
    float avg_threshold = 0.f;        // the config's value (a wakeword's own overrides it)
    float *agg = nullptr, *avg = nullptr;   // [S][n_new]
    uint32_t *fix = nullptr;          // DtwWork::fix, as BankScore::fix
};
hipError_t launch_dtw_bank_stream(hipStream_t st, const BankDev &b, const BankStreamScore &q);

// ---- a bank that changes (rp_bank_put.hip).  One put prepares n_rows template rows of n_entries new entries, as put_rows of Bank::create does
// on the host: row r of the call belongs to the entry e with erow[e] <= r < erow[e + 1] (erow [n_entries + 1], the last = n_rows), is read
// from src + (esrc[e] + r - erow[e]) * K and written to unit / raw + r * K (the caller passes the pool tail).  flags [wakewords of the call],
// zero before: the kernel ORs in what the host decides on before it commits anything.  All device pointers.
constexpr uint32_t kBankPutNotFinite = 1u, kBankPutRefOnly = 2u;
struct BankPut {
    const float *src = nullptr;
    const long long *erow = nullptr, *esrc = nullptr;
    const int32_t *eww = nullptr;     // [n_entries] the wakeword of the call an entry belongs to
    size_t n_entries = 0, n_rows = 0;
    int K = 0;
    float *unit = nullptr, *raw = nullptr;
    uint32_t *flags = nullptr;
};
hipError_t launch_bank_put(hipStream_t st, const BankPut &p);
// Growth and compaction of the row pools: live entry e has len[e] rows at row src_row[e] of the old pools and gets row dst_row[e] of the new.
struct BankMove {
    const float *unit_old = nullptr, *raw_old = nullptr;
    float *unit_new = nullptr, *raw_new = nullptr;
    const long long *src_row = nullptr, *dst_row = nullptr;
    const int32_t *len = nullptr;
    size_t n_entries = 0;
    int K = 0;
};
hipError_t launch_bank_move(hipStream_t st, const BankMove &m);

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE attribute of a kernel: a process that drives several GPUs
// (one rp_ctx per device) has to set it on each of them.  Sets it once per (current device, kernel), thread-safe.
hipError_t allow_dynamic_lds(const void *kernel, int bytes);

enum KernelId { kKernelMfcc = 0, kKernelDtw = 1, kKernelAggregate = 2, kKernelScan = 3, kKernelMlp = 4, kKernelResample = 5, kKernelCount = 6 };

// Sample-rate converter plan (rp_resampler.cpp): out[j] = sum_n x2[n] * g2t[j][n], x2 = previous | current input frame
struct ResamplerDev {
    int fs_in = 0, fi = 0, fo = 0, kpad = 0;  // input rate, input / output frame length, 2*fi rounded up to 16
    const float *g2t = nullptr;                // [fo][kpad]
    const float *fft48 = nullptr;              // 48 kHz only: twiddles + filter spectrum of resample48_fft_kernel
};

// table block of resample48_fft_kernel, offsets in float2 units (rp_resampler.cpp fills it)
constexpr int kR48OffTw240 = 0, kR48OffTw480 = 240, kR48OffTwc = 480, kR48OffW960c = 480 + 6 * 480, kR48OffHf = kR48OffW960c + 256,
              kR48TableLen = kR48OffHf + 480;

struct ScanConfig {
    float threshold, avg_threshold;
    int min_scores, eager, max_len, avg_enabled;
    int fpf = 3;  // MFCC frames per input frame of the stream's encoder: 3 (480 encoded samples) or 4 (640: 11.025 / 22.05 kHz input)
    int stream_base = 0;  // added to the stream index a detection reports (a shard's first global stream, rp_batch_detect_sharded)
};

// the wakewords of one detector in the batched scan (run_wakeword_detectors, src/detector.rs:433-447): per wakeword
// its aggregate scores [S][n_win], avg-template scores (nullptr: gate off) and its own thresholds
constexpr int kScanMaxWakewords = 8;
struct ScanWakewords {
    int n;
    const float *agg[kScanMaxWakewords], *avg[kScanMaxWakewords];
    float threshold[kScanMaxWakewords], avg_threshold[kScanMaxWakewords];
    const int32_t *label[kScanMaxWakewords];  // model wakewords: the winning label of every window (reported instead of j)
    uint32_t *hot = nullptr;                  // [S] from the aggregate pass (AggExtra): 0 = no window of the stream can fire; the scan puts the flags it reads back to 0
};

struct BatchDetection {  // == rp_batch_detection
    int32_t stream, frame, window, counter;
    float avg_score, score;
};

// mfcc2 (optional): a second, packed copy of the frames [S][n_frames][K]
hipError_t launch_mfcc(hipStream_t st, const MfccTablesDev &tb, const float *pcm, size_t S, size_t n_samples,
                       size_t pcm_stride, size_t first_frame, size_t n_frames, size_t out_frame_pitch, float *mfcc,
                       float *mfcc2 = nullptr);

// pcm in one of the reference's sample formats (rp_sample_format: 0 i8, 1 i16, 2 i32, 3 f32), decoded in the kernel
hipError_t launch_mfcc_stream(hipStream_t st, const MfccTablesDev &tb, const void *pcm, int fmt, size_t S, size_t n_chunks,
                              size_t pcm_stride, const float *hist, size_t hist_pitch, float *hist_out, size_t out_frame_pitch,
                              float *mfcc);
hipError_t launch_mfcc_fmt(hipStream_t st, const MfccTablesDev &tb, const void *pcm, int fmt, size_t S, size_t n_samples,
                           size_t pcm_stride, size_t first_frame, size_t n_frames, size_t out_frame_pitch, float *mfcc);

// One scoring call of a template set over S streams x n_win windows: the DTW launches, then the aggregate pass.  The caller describes
// the call; rp_dtw.hip decides which kernels score it, whether the averaged-template gate runs and in which form, whether DTWs may be
// abandoned and whether ScoreMode::Max is folded into the DTW kernel.  mfcc rows have `frame_pitch` frames per stream.
struct Ctx;
struct DtwScore {
    const TemplatesDev *t = nullptr;
    const float *mfcc = nullptr;
    size_t S = 0, frame_pitch = 0, first_win = 0, n_win = 0;
    int band = 0;
    float score_ref = 0.f;
    bool with_avg = false;   // score the averaged template (-> avg); the set has one
    // no per-window score array is part of the call's result: the gate may leave rows unscored (wakeword_comp.rs:85-93) and, in
    // ScoreMode::Max, DTWs that can no longer reach `threshold` may stop with score 0 (GateList::abandon_nc).  Every window
    // that can fire keeps exact scores, so the detections do not change.
    bool detect_only = false;
    float avg_threshold = 0.f, threshold = 0.f;
    int score_mode = 0;   // rp_score_mode
    // outputs: scores [S][n_win][T], avg [S][n_win] (with_avg), agg [S][n_win] (null: no aggregate pass), hot [S] (null: none; else
    // zero before the call, AggExtra), gate_list [1 + S * n_win] words (null: Ctx::ws_list, reserved when the gate runs)
    float *scores = nullptr, *avg = nullptr, *agg = nullptr;
    uint32_t *hot = nullptr, *gate_list = nullptr;
    // How the entry points differ.  Each is kept as it was: harmonising them would change which kernels run.
    bool gate_generic = false;      // the gate also runs behind dtw_generic_kernel (rp_batch_detect_fmt; the others score such sets ungated)
    bool gate_one_stream = true;    // one stream with <= 8 windows is gated too (a live batch of one stream skips the gate's three passes)
    bool fuse_max = false;          // ScoreMode::Max may be folded into the matrix-core kernel (the single-wakeword detect calls)
    bool ragged = false;            // dtw_ragged_kernel's blocks are reserved for the ungated launch (whole-stream batches)
    bool padded_rows = true;        // the frame array ends with slack; false keeps dtw_single_kernel for one stream
    bool timed = true;              // inside the context's kKernelDtw / kKernelAggregate brackets (the single-stream handle times nothing)
};
// false with the error set (hip_ok): "dtw kernel", "dtw kernels (gated)", "dtw_generic_kernel (gated)" or "aggregate_kernel"
bool dtw_score(Ctx &c, const DtwScore &q);

// the single-stream handle's gate-first order (rp_detector.cpp): templates t_first .. t_first + t_count - 1 (index T = the averaged
// template) of a handful of windows of one stream through dtw_single_kernel; hipErrorNotSupported when that kernel does not take the set
hipError_t launch_dtw_single_part(hipStream_t st, const DtwWork &wk, const TemplatesDev &t, const float *mfcc, size_t frame_pitch, size_t first_win, size_t n_win,
                                  size_t out_win_pitch, int band, float score_ref, int t_first, int t_count, float *scores, float *avg);

// Largest template tile the register DTW kernel is built for (0: only the generic kernel applies).
int dtw_register_tile(int K, int band);

// optional extras of the aggregate pass (all null = plain aggregate): gate_avg / gate_threshold -- rows whose averaged-template
// score is below the threshold get aggregate 0 (they were never scored); hot / threshold / n_win -- hot[row / n_win] = 1 for
// streams with a window that can fire (the caller zeroes `hot` first)
struct AggExtra {
    const float *gate_avg = nullptr;
    float gate_threshold = 0.f;
    uint32_t *hot = nullptr;
    float threshold = 0.f;
    size_t n_win = 1;
};
hipError_t launch_aggregate(hipStream_t st, const float *scores, size_t n_rows, int T, int mode, float *agg, AggExtra x = AggExtra{});
// a row of launch_aggregate holds at most kAggMaxT scores (the sort buffer of the percentile modes): false with the error set for a
// reference with more sample templates, asked before anything of the scoring call is launched
constexpr int kAggMaxT = 256;
bool aggregate_fits(int T);

// vad_value [S][n_frames] = mean |mfcc| per frame (launch_vad_value) or nullptr (no VAD);
// vad_mode_value = VADMode::get_value (2 / 2.5 / 3, src/config.rs:140-146)
hipError_t launch_vad_value(hipStream_t st, const float *mfcc, size_t n_frames_total, int K, float *out);
hipError_t launch_vad_value_rows(hipStream_t st, const float *mfcc, size_t S, size_t n, size_t pitch, int K, float *out);
hipError_t launch_scan_multi(hipStream_t st, const ScanWakewords &ww, const float *vad_value, float vad_mode_value, size_t S,
                             size_t n_frames, const ScanConfig &cfg, BatchDetection *det, int32_t *det_ww, int32_t *n_det, int max_det);
// hot (optional): the per-stream flags of the aggregate pass (AggExtra) -- streams whose flag is 0 report no detection unseen
hipError_t launch_scan(hipStream_t st, const float *agg, const float *avg, const float *vad_value, float vad_mode_value,
                       size_t S, size_t n_frames, const ScanConfig &cfg, BatchDetection *det, int32_t *n_det, int max_det,
                       uint32_t *hot = nullptr);
// scan_kernel for a wakeword bank: per stream the window length, thresholds and avg test of its wakeword, rows win_pitch apart (rp_scan.hip)
hipError_t launch_scan_bank(hipStream_t st, const BankDev &b, const int32_t *stream_wakeword, const float *agg, const float *avg, size_t win_pitch,
                            const float *vad_value, float vad_mode_value, size_t S, size_t n_frames, const ScanConfig &cfg, BatchDetection *det,
                            int32_t *n_det, int max_det, uint32_t *hot);

// The gain normaliser's parameters per stream, through the stream's index into a wakeword bank (rp_frontend_batch_bank,
// rp_stream_batch_set_filters_bank): stream s works towards rms_level[w(s)] (fixed_ref for every stream when has_fixed_ref:
// GainNormalizationConfig::gain_ref) over a window of max(ww[w(s)].max_len / 3, 1) chunk levels; an index outside [0, W): no wakeword, gain 1.
struct PerStreamGain {
    const int32_t *stream_wakeword = nullptr;   // [S], device
    const BankWakeword *ww = nullptr;           // [W], device (BankDev::ww)
    const float *rms_level = nullptr;           // [W], device (Bank::rms_level), NaN: none
    int W = 0, has_fixed_ref = 0;
    float fixed_ref = 0.f;
};
// The same parameters for a stream that holds a SET of a bank's entries (wakeword sets, model sets; a model bank's one model is a set of
// one) or rows of TWO banks (mixed sets: references of a wakeword bank and models of a model bank on one detector): stream_targets_kernel
// (rp_gain_targets.hip) folds every stream's rows into one row of a per-stream table -- max_len = Lmax(s), the longest window of the live
// slots; level = the largest non-NaN level of the live slots, NaN when none (on_wakeword_change, src/detector.rs:328-338); idx = s, or -1
// for a stream without a live slot -- and the per-stream gain kernels read that table as they read a bank: PerStreamGain{idx, table,
// level, W = S}.  The mixed scoring and scan kernels read Lmax(s) from it (per->ww).
// One side of it: rows [S][set_size] of indices into a bank of W entries, outside [0, W): an empty slot.  set_size 0 (rows may be null):
// the side is absent.
struct TargetSide {
    const int32_t *rows = nullptr;              // device
    int set_size = 0;
    const BankWakeword *ww = nullptr;           // [W], device: BankDev::ww of a wakeword bank, ModelBank::scan.ww (max_len = L) of a model bank
    const float *level = nullptr;               // [W], device: Bank::rms_level / ModelBank::rms_level, NaN: none
    int W = 0;
};
size_t gain_targets_bytes(size_t S);            // the workspace of S streams
// One short launch over up to two sides (a call over one bank passes TargetSide{} as the second); fills per->stream_wakeword / ww /
// rms_level / W (has_fixed_ref and fixed_ref stay the caller's)
hipError_t launch_stream_targets(hipStream_t st, const TargetSide &first, const TargetSide &second, size_t S, void *workspace, PerStreamGain *per);
// Decode + GainNormalizerFilter + BandPassFilter over whole streams.  ring [S][window_size], rms / gains
// [S][n_samples/480] are device workspaces; biquad coefficients as BandPassFilter::new computes them.
hipError_t launch_frontend(hipStream_t st, const void *pcm, int fmt, size_t S, size_t n_samples, size_t pcm_stride, int gain_on,
                           float rms_level_ref, float min_gain, float max_gain, int window_size, int band_pass, float a0,
                           float a1, float a2, float b1, float b2, float *ring, float *rms, float *gains, float *out,
                           size_t out_stride);
// ... with every stream's own window and reference level; max_window: the bank's largest window, ring [S][max_window]
hipError_t launch_frontend_per_stream(hipStream_t st, const void *pcm, int fmt, size_t S, size_t n_samples, size_t pcm_stride, int gain_on,
                                      const PerStreamGain &per, int max_window, float min_gain, float max_gain, int band_pass, float a0,
                                      float a1, float a2, float b1, float b2, float *ring, float *rms, float *gains, float *out,
                                      size_t out_stride);
// get_rms_level of every chunk alone: rms [S][n_chunks] of rows pcm_stride samples apart
hipError_t launch_chunk_rms(hipStream_t st, const void *pcm, int fmt, size_t S, size_t n_chunks, size_t pcm_stride, float *rms);
// The same filters for the streams of a live batch, state carried from call to call: ONE launch that writes hist rows
// [the last chunk of the previous call (old_hist row + old_off) | the n_chunks new chunks decoded (first of `channels`) and filtered]
// -- launch_stream_stage's row, filtered -- and rms / gains [S][n_chunks] of the new chunks.  filter_state: stream_filter_state_bytes()
// of device memory, zero before a stream's first chunk (biquad x1 x2 y1 y2, gain window head / length, the window ring, by stream).
// At least one of gain_on / band_pass.  per (optional, read with gain_on): every stream its own gain window and reference level; window_size is
// then the capacity of a stream's ring, the largest window any stream may have, and rms_level_ref is not read.
hipError_t launch_stream_filters(hipStream_t st, const void *pcm, int fmt, int channels, size_t S, size_t n_chunks, size_t pcm_stride,
                                 const float *old_hist, size_t old_off, float *hist, size_t hist_pitch, int gain_on,
                                 float rms_level_ref, float min_gain, float max_gain, int window_size, int band_pass, float a0,
                                 float a1, float a2, float b1, float b2, float *filter_state, float *rms, float *gains,
                                 const PerStreamGain *per = nullptr);
size_t stream_filter_state_bytes(size_t S, int window_size);
constexpr size_t kStreamFiltersMaxPitch = (size_t)1 << 25;  // rows (pcm_stride, hist_pitch) must be shorter than this many samples

// Resampler front-end.  Stage: decode + first channel + history -> xs [S][(1+n_chunks)*fi] f32 (prev [S][fi] or
// nullptr = silence before the stream); resample: xs -> out [S][n_chunks*fo].
hipError_t launch_resample_stage(hipStream_t st, const void *pcm, int fmt, int channels, size_t S, size_t n_chunks, int fi,
                                 size_t pcm_stride, const float *prev, float *xs);
hipError_t launch_resample48(hipStream_t st, const float *tables, const void *pcm, int fmt, int channels, size_t pcm_stride,
                             int has_hist, const float *prev, float *prev_out, size_t S, size_t n_chunks, float *out,
                             size_t out_stride);
bool resample_reads_in_place(const ResamplerDev &rs, const void *pcm, int fmt, size_t pcm_stride, const float *out, size_t out_stride);
hipError_t launch_resample_in_place(hipStream_t st, const ResamplerDev &rs, const void *pcm, int fmt, int channels, size_t pcm_stride,
                                    const float *prev, float *prev_out, size_t S, size_t n_chunks, float *out, size_t out_stride);
hipError_t launch_resample(hipStream_t st, const ResamplerDev &rs, const float *xs, size_t S, size_t n_chunks, float *out,
                           size_t out_stride);

// streaming batches (state carried between calls; rp_stream_batch.cpp)
hipError_t launch_stream_stage(hipStream_t st, const void *pcm, int fmt, int channels, size_t S, size_t n_new, size_t pcm_stride,
                               const float *old_hist, size_t old_off, float *hist, size_t hist_pitch);
hipError_t launch_carry_rows(hipStream_t st, const float *src, size_t S, size_t src_pitch, size_t src_off, size_t count, float *dst,
                             size_t dst_pitch);
hipError_t launch_stream_state_init(hipStream_t st, void *state, size_t S);
size_t stream_state_bytes();
hipError_t launch_stream_state_reset(hipStream_t st, void *state, size_t S, long long stream, long long resume);
// the same for streams first .. first + n - 1 (first + n <= S)
hipError_t launch_stream_state_reset_range(hipStream_t st, void *state, size_t S, size_t first, size_t n, long long resume);
// the state machine over this call's n_new frames for a detector that holds 1..8 wakewords (references and / or models); det_ww /
// det_label (optional): the wakeword a detection belongs to and, when that wakeword is a model, its label index (else -1)
hipError_t launch_scan_stream_multi(hipStream_t st, const ScanWakewords &ww, const float *vad_value, float vad_mode_value, size_t S,
                                    long long f0, int n_new, const ScanConfig &cfg, void *state, BatchDetection *det, int32_t *det_ww,
                                    int32_t *det_label, int32_t *n_det, int max_det);
// the same state machine for a batch over a wakeword bank: per stream the window length, countdown, thresholds and avg test of its own
// wakeword (as launch_scan_bank) over agg / avg [S][n_new]; det_ww: the stream's bank index, det_label: -1 (both optional)
hipError_t launch_scan_bank_stream(hipStream_t st, const BankDev &b, const int32_t *stream_wakeword, const float *agg, const float *avg,
                                   const float *vad_value, float vad_mode_value, size_t S, long long f0, int n_new, const ScanConfig &cfg,
                                   void *state, BatchDetection *det, int32_t *det_ww, int32_t *det_label, int32_t *n_det, int max_det,
                                   const int32_t *label = nullptr);   // label [S][n_new] (a model bank's batch): det_label is the label of the detection's best window

// ---- wakeword sets (rp_dtw_set.hip, rp_scan_sets.hip): stream s holds up to kScanMaxWakewords wakewords of a bank, stream_wakewords
// [S][set_size] (outside [0, W): an empty slot) -- a `Rustpotter` with several add_wakeword calls.  Its window is Lmax(s) frames, the longest
// of its set; every wakeword scores the oldest frames of it.
// One scoring call over whole recordings; the BankScore fields mean what they mean there.  Stream s has n_win_s = n_frames - Lmax(s) + 1 windows.
struct BankSetScore {
    const float *mfcc = nullptr;      // [S][n_frames][K]
    size_t S = 0, n_frames = 0, win_pitch = 0;
    const int32_t *stream_wakewords = nullptr;    // [S][set_size]
    int set_size = 0;
    int band = 0, score_mode = 0;
    float score_ref = 0.f;
    int avg_mode = 0, gate = 0;
    float threshold = 0.f, avg_threshold = 0.f;
    // the proposal of every window, [S][win_pitch] each (all three or none): the best passing aggregate, its averaged-template score, its
    // bank index (-1: no wakeword proposes; the first slot of equals wins); zeros / -1 behind a stream's windows
    float *best = nullptr, *best_avg = nullptr;
    int32_t *best_ww = nullptr;
    // the scores slot by slot, [S][set_size][win_pitch] (optional; slot_avg only with slot_agg): zeros behind a stream's windows and in empty slots
    float *slot_agg = nullptr, *slot_avg = nullptr;
    uint32_t *hot = nullptr;          // [S] (optional), zero before the call: raised for streams with a proposal
    uint32_t *fix = nullptr;          // DtwWork::fix
};
// built for dtw_register_tile(K, band) > 0, as launch_dtw_bank
hipError_t launch_dtw_set(hipStream_t st, const BankDev &b, const BankSetScore &q);
// One call of a live-stream batch over sets: q as for launch_dtw_bank_stream with q.stream_wakeword [S][set_size] and q.agg / q.avg
// [S][set_size][n_new]; the window of stream s that ends at a new frame starts Lmax(s) - 1 frames before it.  table (optional): a batch
// over mixed sets (mfcc_size 16 only) -- the COMBINED Lmax(s) of the per-stream table in the place of the set's own, with max_window the
// longest window any stream of the batch may have (its history + 1); without it max_window is not read
hipError_t launch_dtw_set_stream(hipStream_t st, const BankDev &b, const BankStreamScore &q, int set_size, const BankWakeword *table = nullptr,
                                 int max_window = 0);
// the state machine of a stream that holds a set over the proposal rows of launch_dtw_set (window f - Lmax(s) + 1 of rows win_pitch apart);
// det_ww (optional): the bank index of each detection's wakeword.  `hot` as in launch_scan_bank.
hipError_t launch_scan_set(hipStream_t st, const BankDev &b, const int32_t *stream_wakewords, int set_size, const float *best, const float *best_avg,
                           const int32_t *best_ww, size_t win_pitch, const float *vad_value, float vad_mode_value, size_t S, size_t n_frames,
                           const ScanConfig &cfg, BatchDetection *det, int32_t *det_ww, int32_t *n_det, int max_det, uint32_t *hot);
// ... on live streams over the slot scores agg / avg [S][set_size][n_new] of launch_dtw_set_stream: per frame the best proposal of the stream's
// slots, each with its own thresholds (bank_lane); det_ww: the winner's bank index, det_label: -1 (both optional)
hipError_t launch_scan_set_stream(hipStream_t st, const BankDev &b, const int32_t *stream_wakewords, int set_size, const float *agg,
                                  const float *avg, const float *vad_value, float vad_mode_value, size_t S, long long f0, int n_new,
                                  const ScanConfig &cfg, void *state, BatchDetection *det, int32_t *det_ww, int32_t *det_label, int32_t *n_det,
                                  int max_det);

hipError_t launch_synth(hipStream_t st, uint64_t seed, uint64_t first_stream, size_t S, size_t n_samples,
                        size_t pcm_stride, float *pcm);

// Enrolment (rp_average.hip).  MfccNormalizer::normalize over whole samples: sample s owns the first nf[s] frames of raw
// [S][frame_pitch][K]; its normalised rows go to out + dst_row[s] * K.
hipError_t launch_normalize_samples(hipStream_t st, const float *raw, size_t S, size_t frame_pitch, int K, const int32_t *nf,
                                    const int64_t *dst_row, float *out);
// MfccAverager::average for many wakewords: wakeword w folds the templates first[w] .. first[w] + count[w] - 1 in that order (the first is
// the origin); template t is lens[t] rows of K floats at feats + row_off[t] * K; the result (lens[first[w]] rows) goes to avg +
// out_row[w] * K.  All device pointers.
struct AverageBatch {
    const float *feats = nullptr;
    const int32_t *lens = nullptr, *first = nullptr, *count = nullptr;
    const int64_t *row_off = nullptr, *out_row = nullptr;
    float *avg = nullptr;
    int K = 0;
};
// What a workgroup keeps in LDS for an origin of m rows and frames of up to n: both templates, their norms, the path's runs and --
// lds_matrix -- the m x n cost matrix; average_matrix_floats: the matrix alone (a workgroup's workspace slice otherwise).
size_t average_matrix_floats(int m, int n);
size_t average_lds_bytes(int m, int n, int K, bool lds_matrix);
// Two workgroups per CU share its 160 KB: a wakeword whose average_lds_bytes(.., true) is within this keeps its matrix in LDS
constexpr size_t kAvgLdsBudget = 80 * 1024;
// One launch over the listed wakewords (`blocks` workgroups stride over them).  lds_bytes: the largest average_lds_bytes of the list;
// ws: blocks x ws_slice floats (the matrices of a launch with lds_matrix false).
hipError_t launch_average(hipStream_t st, const AverageBatch &b, const int32_t *list, size_t n_list, bool lds_matrix, size_t lds_bytes,
                          unsigned blocks, float *ws, size_t ws_slice);

// x [B][dims[0]] -> out [B][dims[n_layers]]; W/Bv device pointers per layer.
// MfccNormalizer::normalize of windows [w, w+L) flattened row-major to x [n_win][L*K]
// (WakewordNN::run_detection, src/wakewords/nn/wakeword_nn.rs:139-149,268-273).
hipError_t launch_normalize_windows(hipStream_t st, const float *mfcc, size_t first_win, size_t n_win, int L, int K,
                                    float *x);

// Device-resident wakeword model (src/wakewords/nn/wakeword_nn.rs:305-389): layer 1 padded for
// the MFMA kernels, the small tail layers packed for the per-row epilogue.
struct MlpDev {
    int n_layers = 0;
    int dims[5] = {0, 0, 0, 0, 0};
    int nt = 0;            // 16-column tiles of layer 1 (1, 2, 5 or 9)
    int kpad = 0;          // dims[0] rounded up to 128
    float *w1f = nullptr;  // [16*nt][kpad] f32, zero padded
    void *w1h = nullptr;   // [16*nt][kpad] bf16, zero padded
    void *w1s = nullptr;   // [2][16*nt][kpad] f16: the two parts of the weights' f16 split (kMlpF16x2), zero padded
    void *w1t = nullptr;   // [3][16*nt][kpad] bf16: the three parts of the weights' exact bf16 split (kMlpBf16x3), zero padded
    void *wwin = nullptr;  // mfcc_size 16, layer 1 <= 160 wide: the same two parts in the order the lanes of mlp_windows_kernel (<= 32 wide) /
                           // mlp_windows_wide_kernel read them, [frame f][32-output tile q][part][k-half h][output j < 32][8 k = 16 f + 8 h ..] f16
    void *wwin3 = nullptr; // the same in three bf16 parts (kMlpBf16x3): [frame f][32-output tile q][part 3][k-half h][output j < 32][8 k]
    float *b1 = nullptr;   // [16*nt]
    float *tail = nullptr; // layers 2..n: W [out][in] then b [out], concatenated
    int tail_floats = 0;
};
// Operand forms of layer 1 on the matrix cores, the PREC of mlp_mfma_kernel / mlp_stream_kernel (mlp_route maps RP_MLP_* onto them):
// kMlpF32: the f32 matrix instructions (RP_MLP_F32_STRICT; also the second pass of kMlpF16x2, and RP_MLP_F32 on a model whose three-part
// weight groups do not fit the LDS).  kMlpBf16: inputs rounded to bf16 (RP_MLP_BF16).
// kMlpF16x2 (RP_MLP_F32_FAST): inputs and weights as f16 two-way splits (x = x0 + x1, w = w0 + w1, 22 significant bits each;
// x0 w0 + x1 w0 + x0 w1, f32 accumulate: the dropped x1 w1 is 2^-22 of a product).  A row with a feature beyond the f16 range (|x| > 65504,
// or not finite) is listed in redo (Ctx::mlp_redo: [2 + B] words, redo[0] = rows listed, redo[1] = workgroups of the second pass done, both
// zero between calls) and computed again by a second pass with the f32 matrix instructions -- rp_mlp_forward_batch never answers NaN for
// finite input.
// kMlpBf16x3 (RP_MLP_F32): inputs and weights as THREE bf16 parts each (exact), six of the nine partial products, f32 accumulate.  No range
// limit, no second pass.
enum { kMlpF32 = 0, kMlpBf16 = 1, kMlpF16x2 = 2, kMlpBf16x3 = 5 };
bool mlp_mfma_fits(const MlpDev &m);   // mlp_mfma_kernel's LDS fits a CU (else: the per-layer kernel)
// The same forward for dense rows with the rows streamed through LDS by LDS-DMA in whole 128-byte lines (rp_mlp_stream.hip):
// layer-1 widths <= 32, row pitch a multiple of 64 bytes, x 16-byte aligned (mlp_stream_supported).  The plan holds the
// layer-1 weights in MFMA-fragment order and the line phases of the rows (Model::stream_plan).
struct MlpStreamPlan {
    const void *wimg = nullptr;                // [k-step m][...] k-step m = k in [32m, 32m+32), zero padded; see Model::stream_plan
    int q[2] = {0, 0};                         // even / odd rows: 16-byte chunks between a row's start and the line start below it
    int units = 0;                             // 64-k steps per row (2 lines of 128 bytes)
    int par = 0;                               // 1: even and odd rows differ in phase -- a workgroup takes rows of one parity
    int nbt = 0;                               // workgroup tiles: 128 rows (256-row span of one parity when par)
};
bool mlp_stream_supported(const MlpDev &m, const float *x, int precision);
hipError_t launch_mlp_stream(hipStream_t st, const MlpDev &m, const MlpStreamPlan &p, const float *x, size_t B, int precision, float *out,
                             int n_cu, uint32_t *redo, const char **build = nullptr);   // the streaming pass alone (kMlpF16x2: mlp_forward
                                                                                       // runs the second pass).  *build: "" for the build the
                                                                                       // launcher picks by itself, else the ring depth and waves
                                                                                       // RP_MLP_STREAM_DEPTH / RP_MLP_STREAM_WAVES moved it to
// The rows may also be windows of L = dims[0]/K frames read IN PLACE from mfcc [S][frame_pitch][K] (window w of stream s starts at frame
// s * frame_pitch + w): the window mean (MfccNormalizer::normalize) is taken out after layer 1, W.(f - mu) = W.f - sum_k mu[k] * wsum[o][k],
// wsum[o][k] = sum_i W[o][i*K + k] (Model::wsum_for); mean [S*n_win][K] from launch_window_means.
hipError_t launch_window_means(hipStream_t st, const float *mfcc, size_t S, size_t n_frames, size_t n_win, int L, int K, float *mean);

// One wakeword-model forward.  The caller describes the call; mlp_route (rp_mlp.hip) decides which kernels run it, in which operand form.
struct Model;
struct MlpForward {
    Model *m = nullptr;
    int precision = 0;               // rp_mlp_precision
    const float *x = nullptr;        // dense rows x [B][dims[0]], or with `windows` the frames: S x n_win windows read in place
    size_t B = 0, S = 0, n_win = 0, frame_pitch = 0;
    bool windows = false;
    int K = 0;
    const float *mean = nullptr, *wsum = nullptr;
    float *out = nullptr;            // logits [rows][dims[n_layers]]
    float *scratch[2] = {nullptr, nullptr};   // the per-layer kernel's intermediates, [rows][widest layer] each (no mfma_ok only)
    // How the callers differ.  Each is kept as it was: harmonising them would change which kernels run.
    bool allow_stream = true;        // dense rows may take mlp_stream_kernel (the single-stream handle never does)
    bool report = true;              // set Ctx::last_mlp_kernel (live batches' in-place windows and the single-stream handle leave it)
    bool timed = true;               // inside the context's kKernelMlp bracket (the single-stream handle times nothing)
};
// false with the error set (hip_ok): "mlp_mfma_kernel" or "mlp_layer_kernel"
bool mlp_forward(Ctx &c, const MlpForward &q);

// WakewordModelTrain (src/wakewords/nn/wakeword_model_train.rs:204-209): act[l] / dz[l] are [B][dims[l+1]] device buffers
hipError_t launch_train_forward(hipStream_t st, const float *x, size_t B, int n_layers, const int *dims, float *const *W,
                                float *const *Bv, float *const *act);
hipError_t launch_train_step(hipStream_t st, const float *x, const int32_t *labels, size_t B, int n_layers, const int *dims,
                             float *const *W, float *const *Bv, float *const *act, float *const *dz, float lr, float *loss_rows);
// The same for many models in one launch (train_batch_kernel, rp_train_batch.hip): one workgroup per job, the epochs inside
// the kernel.  A job's state lies in its own pieces of one workspace `ws` of floats; every offset counts floats from ws and is a multiple
// of 4 (16 bytes).  x [B][dims[0]] and xt [Bt][dims[0]]: train and test rows; labels [B] int32; w[l] [dims[l+1]][dims[l]] and b[l]
// [dims[l+1]]; act[l] [max(B, Bt)][dims[l+1]]; dz[l] [B][dims[l+1]]; loss [B]: the rows of the last epoch's loss; tlog [Bt][dims[n_layers]]:
// the test rows' logits under the weights as the launch leaves them.
constexpr int kTrainBatchThreads = 1024;
constexpr int kTrainMaxLayers = 4;
struct TrainJob {
    int n_layers, B, Bt, pad0;
    int dims[kTrainMaxLayers + 1], pad1[3];
    long long x, xt, labels, loss, tlog, pad2;
    long long w[kTrainMaxLayers], b[kTrainMaxLayers], act[kTrainMaxLayers], dz[kTrainMaxLayers];
};
static_assert(sizeof(TrainJob) % 16 == 0, "the job table precedes 16-byte aligned rows in the workspace");
// `epochs` steps of every job (the bits of launch_train_step, whatever the cut into launches), then, with test_forward, the forward of
// the test rows into tlog.  grid workgroups walk the n_jobs jobs; nothing but the workgroup of a job touches its pieces.
hipError_t launch_train_batch(hipStream_t st, const TrainJob *jobs, size_t n_jobs, unsigned grid, float *ws, float lr, int epochs,
                              int test_forward);
// WakewordNN::run_detection (src/wakewords/nn/wakeword_nn.rs:39-159) over whole batches: windows of L frames cut from
// mfcc [S][frame_pitch][K] and mean-normalised into rows (first_row .. first_row+n_rows of the S*n_win windows), and the
// label / score logic on the logits: agg = score where the detection is valid (label != none, score >= threshold,
// avg_score >= avg_threshold) else -2, avg = avg_score, label = arg-max label.
hipError_t launch_normalize_windows_batch(hipStream_t st, const float *mfcc, size_t frame_pitch, size_t n_win, size_t first_row,
                                          size_t n_rows, int L, int K, float *x);
hipError_t launch_nn_score(hipStream_t st, const float *logits, size_t n_rows, int n_labels, int none_index, float score_ref10,
                           int calc_avg, float threshold, float avg_threshold, float *agg, float *avg, int32_t *label,
                           uint32_t *hot = nullptr, size_t rows_per_stream = 0);  // hot: a flag per stream (zeroed by the caller) raised by every window that passed

// ---- model bank (rp_model_bank.cpp; kernels in rp_mlp_windows.hip, scoring in rp_mlp.hip): W wakeword models resident on the device, stream s runs its own model
// stream_model[s] (outside [0, W): none).  The bank holds copies of what mlp_windows_kernel's three-part form reads of a model, in pools:
// the lane-ordered image MlpDev::wwin3, b1, wsum for mfcc_size 16 and the packed tail; a descriptor per model says where.
struct ModelBankEntry {
    long long wimg;          // first 16-byte piece of its image in ModelBankDev::wimg
    long long b1, wsum, tail;   // first float in the three float pools
    int L, n1p;              // window length (train_size); rows of b1 / wsum (16 or 32)
    int n_layers, d1, d2, d3;
    int tail_floats, n_labels, none_index, pad;
};
struct ModelBankDev {
    int W = 0, label_pitch = 0;           // label_pitch: the largest label count
    const ModelBankEntry *e = nullptr;    // [W]
    const void *wimg = nullptr;           // 16-byte pieces
    const float *b1 = nullptr, *wsum = nullptr, *tail = nullptr;
};
// The shape of one call's launch: NT = the most tiles a workgroup of the call owns, bps = the most workgroups a stream has, LDS bytes for the
// largest staging.  model_bank_shape works it out from the window lengths / tail sizes of the models the call may use.
struct ModelBankShape { int nt = 0; unsigned bps = 0; size_t lds = 0; };
void model_bank_shape_add(ModelBankShape *sh, size_t n_frames, int L, int tail_floats);
// window means of every stream's own window length, mean [S][win_pitch][16] (the sums of launch_window_means, frame order)
hipError_t launch_window_means_bank(hipStream_t st, const ModelBankDev &b, const int32_t *stream_model, const float *mfcc, size_t S, size_t n_frames,
                                    size_t win_pitch, float *mean);
// logits [S][win_pitch][label_pitch], zeroed here: row (s, w) gets the labels of s's model for w < n_win(s)
hipError_t launch_mlp_windows_bank(hipStream_t st, const ModelBankDev &b, const ModelBankShape &sh, const int32_t *stream_model, const float *mfcc,
                                   size_t S, size_t n_frames, const float *mean, size_t win_pitch, float *logits);
// launch_nn_score with the label count and none_index of each row's model; rows without a window: agg -2, avg 0, label -1
hipError_t launch_nn_score_bank(hipStream_t st, const ModelBankDev &b, const int32_t *stream_model, const float *logits, size_t S, size_t n_frames,
                                size_t win_pitch, float score_ref10, int calc_avg, float threshold, float avg_threshold, float *agg, float *avg,
                                int32_t *label, uint32_t *hot);
// det_label [S][max_det] = the label of each detection's window (label [S][win_pitch]), 0 behind a stream's detections
hipError_t launch_model_bank_labels(hipStream_t st, const BatchDetection *det, const int32_t *n_det, const int32_t *label, size_t S, size_t win_pitch,
                                    int max_det, int32_t *det_label);

// ---- a model bank that changes (rp_model_bank_put.hip).  One put prepares the pool entries of n models from their raw f32 parameters on the
// device -- per layer weights [out][in] and biases [out]: an rp_model's plain copies, a staged upload or the training workspace -- with the bits
// Model::create + Model::wsum_for(16) + ModelBank::create give on the host: the three-part layer-1 image (bf16_split3 of rp_ctx.cpp, operation
// for operation), b1, wsum (f64 sums in frame order) and the packed tail.  `e` says where in the pools (the caller passes the pool bases; the
// entries lie in the pool tails, which nothing in flight reads).  flags [n], zero before: the kernel ORs in what the host decides on before it
// commits anything.  All device pointers.
constexpr uint32_t kModelPutNotFinite = 1u;
struct ModelPutItem {
    const float *w[3], *b[3];   // layers 1..n_layers; 16-byte aligned
    ModelBankEntry e;
};
struct ModelBankPut {
    const ModelPutItem *items = nullptr;
    size_t n = 0;
    int max_L = 0, max_tail = 0;   // the longest window and the largest tail pitch among the items: the launch's workgroups per model
    void *wimg = nullptr;
    float *b1 = nullptr, *wsum = nullptr, *tail = nullptr;
    uint32_t *flags = nullptr;
};
hipError_t launch_model_bank_put(hipStream_t st, const ModelBankPut &p);
// Growth and compaction of the four pools: live model i has its entries where from[i] says in the old pools and gets those of to[i] in the new.
struct ModelBankMove {
    const ModelBankEntry *from = nullptr, *to = nullptr;
    size_t n = 0;
    const void *wimg_old = nullptr;
    const float *b1_old = nullptr, *wsum_old = nullptr, *tail_old = nullptr;
    void *wimg_new = nullptr;
    float *b1_new = nullptr, *wsum_new = nullptr, *tail_new = nullptr;
};
hipError_t launch_model_bank_move(hipStream_t st, const ModelBankMove &m);

// ---- live batches over a model bank (rp_mlp_bank_stream.hip; rp_stream_batch_new_model_bank): the n_new new windows of every stream, frame rows
// [S][cap][16] with the first new frame at `fill` (>= max_L - 1, the bank's longest window, and fill + n_new <= cap); the window of stream s
// that ends at new frame i starts L(s) - 1 frames before it.  mean [S][n_new][16], logits [S][n_new][label_pitch] (every row written: zeros
// behind a model's labels and for a stream without a model).  Row by row the arithmetic of mlp_mfma_kernel<NT, kMlpBf16x3> in window mode.
hipError_t launch_window_means_bank_stream(hipStream_t st, const ModelBankDev &b, int max_L, const int32_t *stream_model, const float *frames, size_t S,
                                           size_t cap, size_t fill, size_t n_new, float *mean);
hipError_t launch_mlp_bank_stream(hipStream_t st, const ModelBankDev &b, int max_L, const int32_t *stream_model, const float *frames, size_t S,
                                  size_t cap, size_t fill, size_t n_new, const float *mean, float *logits);
// launch_nn_score_bank over those rows: logits [S][n_new][label_pitch] -> agg / avg / label [S][n_new]; a stream without a model: -2, 0, -1
hipError_t launch_nn_score_bank_stream(hipStream_t st, const ModelBankDev &b, const int32_t *stream_model, const float *logits, size_t S, size_t n_new,
                                       float score_ref10, int calc_avg, float threshold, float avg_threshold, float *agg, float *avg, int32_t *label);

// ---- model sets (rp_mlp_model_set.hip, rp_scan_sets.hip): stream s holds up to kScanMaxWakewords models of a model bank, sets
// [S][set_size] (outside [0, W): an empty slot) -- a `Rustpotter` with several add_wakeword calls of models.  Its window is Lmax(s) frames, the
// longest train_size of its live slots; slot j scores the oldest L_j frames of it.
// Whole recordings: stream s has n_win_s = n_frames - Lmax(s) + 1 windows.  The launch shape of the models a call uses: one
// model_set_shape_add per (Lmax of a stream, a model of its set).
void model_set_shape_add(ModelBankShape *sh, size_t n_frames, int lmax, int L, int tail_floats);
// mean [S][set_size][win_pitch][16]: row (s, j, w) is the mean of the L_j frames from frame w of stream s
hipError_t launch_window_means_model_set(hipStream_t st, const ModelBankDev &b, const int32_t *sets, int set_size, const float *mfcc, size_t S,
                                         size_t n_frames, size_t win_pitch, float *mean);
// logits [S][set_size][win_pitch][label_pitch], zeroed here: row (s, j, w) gets the labels of model sets[s][j] for w < n_win_s
hipError_t launch_mlp_windows_model_set(hipStream_t st, const ModelBankDev &b, const ModelBankShape &sh, const int32_t *sets, int set_size,
                                        const float *mfcc, size_t S, size_t n_frames, const float *mean, size_t win_pitch, float *logits);
// the proposal of every window, [S][win_pitch] each: the best passing score over the live slots (-2: nobody proposes; the first slot of
// equals wins), its average score, the winner's bank index (-1) and label (-1).  hot [S] (optional) as in launch_nn_score_bank.
hipError_t launch_nn_score_model_set(hipStream_t st, const ModelBankDev &b, const int32_t *sets, int set_size, const float *logits, size_t S,
                                     size_t n_frames, size_t win_pitch, float score_ref10, int calc_avg, float threshold, float avg_threshold,
                                     float *best, float *best_avg, int32_t *best_ww, int32_t *best_label, uint32_t *hot);
// the state machine over those rows; b: ModelBank::scan.  det_ww / det_label (optional): each detection's bank index and label
hipError_t launch_scan_model_set(hipStream_t st, const BankDev &b, const int32_t *stream_models, int set_size, const float *best,
                                 const float *best_avg, const int32_t *best_ww, const int32_t *best_label, size_t win_pitch, const float *vad_value,
                                 float vad_mode_value, size_t S, size_t n_frames, const ScanConfig &cfg, BatchDetection *det, int32_t *det_ww,
                                 int32_t *det_label, int32_t *n_det, int max_det, uint32_t *hot);
// Live: frames, cap, fill, n_new and max_L as for launch_mlp_bank_stream; the window of stream s that ends at new frame i starts Lmax(s) - 1
// frames before it for every slot.  mean [S][set_size][n_new][16], logits [S][set_size][n_new][label_pitch] (every row written).
hipError_t launch_window_means_set_stream(hipStream_t st, const ModelBankDev &b, int max_L, const int32_t *sets, int set_size, const float *frames,
                                          size_t S, size_t cap, size_t fill, size_t n_new, float *mean);
hipError_t launch_mlp_set_stream(hipStream_t st, const ModelBankDev &b, int max_L, const int32_t *sets, int set_size, const float *frames, size_t S,
                                 size_t cap, size_t fill, size_t n_new, const float *mean, float *logits);
// agg / avg / label [S][set_size][n_new] slot by slot; an empty slot: -2, 0, -1
hipError_t launch_nn_score_set_stream(hipStream_t st, const ModelBankDev &b, const int32_t *sets, int set_size, const float *logits, size_t S,
                                      size_t n_new, float score_ref10, int calc_avg, float threshold, float avg_threshold, float *agg, float *avg,
                                      int32_t *label);
// per frame the best proposal of the stream's slots over those rows (b: ModelBank::scan); det_ww: the winner's bank index, det_label: the
// label of the detection's best window
hipError_t launch_scan_model_set_stream(hipStream_t st, const BankDev &b, const int32_t *stream_models, int set_size, const float *agg,
                                        const float *avg, const int32_t *label, const float *vad_value, float vad_mode_value, size_t S, long long f0,
                                        int n_new, const ScanConfig &cfg, void *state, BatchDetection *det, int32_t *det_ww, int32_t *det_label,
                                        int32_t *n_det, int max_det);

// ---- mixed sets (rp_gain_targets.hip, rp_scan_sets.hip): stream s holds a row of wakeword references of a wakeword bank AND a row of models
// of a model bank -- one `Rustpotter` with add_wakeword of both kinds (src/detector.rs:304-346,433-447).  Its window is Lmax(s) frames, the
// longest over the live slots of BOTH rows.
// The proposals of one side of a whole-recording mixed call, rows win_pitch apart: those of launch_dtw_set (label null) or of
// launch_nn_score_model_set.  bank: the side's BankDev (ModelBank::scan for models); set_size 0: the side is absent and nothing is read.
struct MixedProposals {
    BankDev bank;
    const int32_t *rows = nullptr;
    int set_size = 0;
    const float *best = nullptr, *best_avg = nullptr;
    const int32_t *best_ww = nullptr, *best_label = nullptr;
};
// the state machine of a stream that holds a mixed set: Lmax(s) from table (launch_stream_targets), per window the better of the two sides'
// proposals, the reference of equals; a side without a live slot for the stream is not read.  det_ww: the winner's index in ITS OWN bank,
// det_label: the winner's label for a model, -1 for a reference (both optional).  `hot` as in launch_scan_bank.
hipError_t launch_scan_mixed_set(hipStream_t st, const MixedProposals &refs, const MixedProposals &models, const BankWakeword *table, size_t win_pitch,
                                 const float *vad_value, float vad_mode_value, size_t S, size_t n_frames, const ScanConfig &cfg, BatchDetection *det,
                                 int32_t *det_ww, int32_t *det_label, int32_t *n_det, int max_det, uint32_t *hot);
// Live, the model side of a batch over mixed sets (rp_mlp_mixed.hip): launch_window_means_set_stream / launch_mlp_set_stream with the COMBINED
// Lmax(s) of `table` (max_L: the model bank's longest window; max_window: the longest window any stream of the batch may have, its
// history + 1); launch_nn_score_set_stream scores their logits as it is
hipError_t launch_window_means_mixed_stream(hipStream_t st, const ModelBankDev &b, int max_L, int max_window, const int32_t *sets, int set_size,
                                            const BankWakeword *table, const float *frames, size_t S, size_t cap, size_t fill, size_t n_new,
                                            float *mean);
hipError_t launch_mlp_mixed_stream(hipStream_t st, const ModelBankDev &b, int max_L, int max_window, const int32_t *sets, int set_size,
                                   const BankWakeword *table, const float *frames, size_t S, size_t cap, size_t fill, size_t n_new,
                                   const float *mean, float *logits);
// the carried state machine over both sides' slot rows: ragg / ravg [S][ref_size][n_new] under the references' own thresholds (rb: the
// wakeword bank), magg / mavg / mlabel [S][model_size][n_new] where not -2 (mb: ModelBank::scan); a size of 0: the side is absent
hipError_t launch_scan_mixed_set_stream(hipStream_t st, const BankDev &rb, const int32_t *ref_rows, int ref_size, const BankDev &mb,
                                        const int32_t *model_rows, int model_size, const BankWakeword *table, const float *ragg, const float *ravg,
                                        const float *magg, const float *mavg, const int32_t *mlabel, const float *vad_value, float vad_mode_value,
                                        size_t S, long long f0, int n_new, const ScanConfig &cfg, void *state, BatchDetection *det, int32_t *det_ww,
                                        int32_t *det_label, int32_t *n_det, int max_det);

}  // namespace rp
