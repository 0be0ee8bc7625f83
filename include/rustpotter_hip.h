/*
 * rustpotter_hip.h -- C ABI of librustpotter_hip.so, an MI355X (gfx950) HIP
 * implementation of rustpotter v3.0.2's MFCC + DTW wakeword scoring path.
 *
 * The reference has no C ABI of its own; its public surface is the
 * Rust API re-exported in src/lib.rs:8-21.  Every entry point below cites the
 * reference item it replaces (paths relative to the reference root).  A Rust
 * crate binds this header with `extern "C"` (bindings/rustpotter_hip.rs,
 * INTEGRATION.md) and re-exposes the reference's method names unchanged.
 *
 * Conventions (SURVEY.md §8b "Ownership/Errors/Threading"):
 *  - all functions return plain C types; status returns are int: >=0 ok, <0 error;
 *    the message of the last error of the calling thread is rp_last_error()
 *    (the reference returns Result<_, String>).  A NULL handle or a NULL required pointer is
 *    refused with -1 ("null handle" / "null argument"); getters return 0, *_free(NULL) is a no-op.
 *  - the caller owns every input buffer for the duration of the call only;
 *    wakewords are copied into the handle (src/wakewords/comp/wakeword_comp.rs:55-63).
 *  - strings/arrays inside rp_detection are owned by the handle and stay valid
 *    until the next call on that handle.
 *  - handles are NOT thread-safe (reference: every method takes &mut self); distinct
 *    handles are independent.
 *  - nothing in this library falls back to the CPU: without a usable HIP device
 *    rp_new / rp_ctx_new fail with an error.
 */
#ifndef RUSTPOTTER_HIP_H
#define RUSTPOTTER_HIP_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ config */
/* src/audio/audio_types.rs:4-9 */
typedef enum { RP_SAMPLE_I8 = 0, RP_SAMPLE_I16 = 1, RP_SAMPLE_I32 = 2, RP_SAMPLE_F32 = 3 } rp_sample_format;
/* src/audio/audio_types.rs:52-56 */
typedef enum { RP_ENDIAN_BIG = 0, RP_ENDIAN_LITTLE = 1, RP_ENDIAN_NATIVE = 2 } rp_endianness;
/* src/config.rs:86-96 (declaration order) */
typedef enum {
    RP_SCORE_AVERAGE = 0, RP_SCORE_MAX = 1, RP_SCORE_MEDIAN = 2, RP_SCORE_P25 = 3, RP_SCORE_P50 = 4,
    RP_SCORE_P75 = 5, RP_SCORE_P80 = 6, RP_SCORE_P90 = 7, RP_SCORE_P95 = 8
} rp_score_mode;
/* src/config.rs:134-138; RP_VAD_NONE == Option::None */
typedef enum { RP_VAD_NONE = 0, RP_VAD_EASY = 1, RP_VAD_MEDIUM = 2, RP_VAD_HARD = 3 } rp_vad_mode;

/* src/config.rs:10-19 AudioFmt */
typedef struct {
    size_t sample_rate;
    rp_sample_format sample_format;
    uint16_t channels;
    rp_endianness endianness;
} rp_audio_fmt;

/* src/config.rs:172-191 DetectorConfig */
typedef struct {
    float avg_threshold;
    float threshold;
    size_t min_scores;
    bool eager;
    float score_ref;
    uint16_t band_size;
    rp_score_mode score_mode;
    rp_vad_mode vad_mode;
} rp_detector_config;

/* src/config.rs:32-42 GainNormalizationConfig (gain_ref: Option<f32>) */
typedef struct {
    bool enabled;
    bool has_gain_ref;
    float gain_ref;
    float min_gain;
    float max_gain;
} rp_gain_normalization_config;

/* src/config.rs:55-62 BandPassConfig */
typedef struct {
    bool enabled;
    float low_cutoff;
    float high_cutoff;
} rp_band_pass_config;

/* src/config.rs:75-82 FiltersConfig */
typedef struct {
    rp_gain_normalization_config gain_normalizer;
    rp_band_pass_config band_pass;
} rp_filters_config;

/* src/config.rs:212-219 RustpotterConfig */
typedef struct {
    rp_audio_fmt fmt;
    rp_detector_config detector;
    rp_filters_config filters;
} rp_config;

/* RustpotterConfig::default(), src/config.rs:20-29,43-52,63-71,192-207 */
void rp_config_default(rp_config *out);

/* --------------------------------------------------------------- detection */
/* src/detector.rs:488-501 RustpotterDetection.  `scores` is the HashMap<String,f32>
 * flattened to parallel arrays (template file names for references, label names
 * for models). */
typedef struct {
    const char *name;
    float avg_score;
    float score;
    size_t n_scores;
    const char *const *score_names;
    const float *scores;
    size_t counter;
    float gain;
} rp_detection;

/* ------------------------------------------- single-stream `Rustpotter` mirror */
typedef struct rp_detector rp_detector;

/* Rustpotter::new, src/detector.rs:95-141.  config->fmt.sample_rate may be any rate AudioEncoder::new
 * (src/audio/encoder.rs:63-83) accepts whose 16 kHz output frame is 480 or 640 samples -- every standard
 * audio rate: 8 / 16 / 32 / 48 / 96 kHz and the 44.1 kHz family give 30 ms input frames (3 MFCC frames per
 * call), 11.025 / 22.05 kHz give 40 ms frames (640 encoded samples, 4 MFCC frames per call).  Input that is
 * not 16 kHz goes through the device resampler (rubato FftFixedInOut restated);
 * rp_get_samples_per_frame() is then the resampler's input frame x channels (1 440 for 48 kHz mono).
 * Errors: "Unsupported sample rate, unable to initialize the resampler" (src/audio/encoder.rs:78) for rate 0
 * and for rates whose output frame has no device kernel (rp_resampler_frame_lengths tells). */
int rp_new(const rp_config *config, rp_detector **out);
void rp_free(rp_detector *d);

/* add_wakeword_from_buffer / _from_file, src/detector.rs:152-176 (WakewordV2 ->
 * WakewordRef -> WakewordModel fall-through, decided on the CBOR map keys). */
int rp_add_wakeword_from_buffer(rp_detector *d, const char *key, const uint8_t *buffer, size_t len);
int rp_add_wakeword_from_file(rp_detector *d, const char *key, const char *path);
/* remove_wakeword / remove_wakewords, src/detector.rs:180-202 */
bool rp_remove_wakeword(rp_detector *d, const char *key);
bool rp_remove_wakewords(rp_detector *d);

/* src/detector.rs:204-229 */
size_t rp_get_samples_per_frame(const rp_detector *d);
size_t rp_get_bytes_per_frame(const rp_detector *d);
/* returns 1 and fills *out if a partial detection exists, else 0 */
int rp_get_partial_detection(const rp_detector *d, rp_detection *out);
float rp_get_rms_level(const rp_detector *d);
float rp_get_gain(const rp_detector *d);
float rp_get_rms_level_ref(const rp_detector *d);

/* process_bytes, src/detector.rs:234-240; process_samples::<T>, :245-254.
 * Return 1 (detection written to *out), 0 (None: also for a wrong buffer length or
 * no wakewords, exactly like the reference), <0 device error. */
int rp_process_bytes(rp_detector *d, const uint8_t *audio_bytes, size_t len, rp_detection *out);
int rp_process_samples_i8(rp_detector *d, const int8_t *samples, size_t n, rp_detection *out);
int rp_process_samples_i16(rp_detector *d, const int16_t *samples, size_t n, rp_detection *out);
int rp_process_samples_i32(rp_detector *d, const int32_t *samples, size_t n, rp_detection *out);
int rp_process_samples_f32(rp_detector *d, const float *samples, size_t n, rp_detection *out);

/* update_config / update_detector_config / update_filters_config / reset,
 * src/detector.rs:257-302 */
int rp_update_config(rp_detector *d, const rp_config *config);
int rp_update_detector_config(rp_detector *d, const rp_detector_config *config);
int rp_update_filters_config(rp_detector *d, const rp_filters_config *config);
void rp_reset(rp_detector *d);

/* Result<_, String> error text of the calling thread's last failing call */
const char *rp_last_error(void);

/* ------------------------------------------------- batched operator level
 * What the HIP kernels sit behind: the reference's per-frame operators applied to
 * S independent streams at once.  All array arguments are DEVICE pointers unless
 * the context was created with RP_CTX_HOST_POINTERS (then the library stages
 * them through its own device buffers). */
typedef struct rp_ctx rp_ctx;
typedef struct rp_templates rp_templates;

/* RP_CTX_FULL_SCORES: rp_batch_detect* compare every window with every sample template to the end even when the
 * averaged-template gate (avg_threshold != 0, wakeword_comp.rs:85-93) would skip them or the running cost already rules a
 * detection out -- the behaviour of the per-window score outputs, forced for calls that do not ask for them (same
 * detections either way; used to time the paths against each other). */
enum {
    RP_CTX_DEVICE_POINTERS = 0, RP_CTX_HOST_POINTERS = 1, RP_CTX_FULL_SCORES = 2,
    /* the arithmetic of the context's DTW scoring (RP_ARITH_* below; neither bit: RP_ARITH_F32_MATRIX) */
    RP_CTX_ARITH_STRICT_F32 = 4, RP_CTX_ARITH_FAST_SPLIT = 8,
    /* with RP_CTX_ARITH_FAST_SPLIT: references whose templates differ in length also go to the matrix cores (dtw_ragged_kernel) */
    RP_CTX_RAGGED_MATRIX = 16
};

/* device: HIP device ordinal.  Fails (<0) if no HIP device is usable, or when both RP_CTX_ARITH_* bits are set. */
int rp_ctx_new(int device, int flags, rp_ctx **out);
/* The arithmetic of the cosine products of the DTW cost (replaces the implicit "f32" of src/mfcc/comparator.rs:28-48, whose products and
 * sums are f32 -- the config-is-a-struct convention of src/config.rs:172-219, not an environment variable).  The window mean, the norms, the
 * min-plus recurrence, the score and every index are f32 / integer arithmetic in every mode; the modes differ in where the five products of
 * a band cell are formed and how many bits of them are kept:
 *   RP_ARITH_F32_MATRIX (default)  matrix cores, f32-grade: both operands as three bf16 parts (exact: 3 x 8 = an f32's 24 significant bits),
 *       six of the nine partial products accumulated in f32 -- what is dropped is below 2^-22 of a product (2^-25.7 rms; an f32 multiply
 *       rounds by up to 2^-24, 2^-25.3 rms): mfcc_size 5 in chunks of 3..8 templates of one length, mfcc_size 13 / 16 in chunks of up to
 *       four.  Template sets with no such kernel (lengths that occur once or twice, other frame sizes, a band other than 3..5) run the
 *       f32 vector kernels.
 *   RP_ARITH_STRICT_F32            f32 vector FMAs for every product (the "register" kernels), nothing on the matrix cores.
 *   RP_ARITH_FAST_SPLIT            matrix cores with two f16 parts per operand (22 significant bits, one partial product dropped): the
 *       fastest form, NARROWER than the reference's f32 products; scores stay within the 1e-5 parity gate for score_ref >= 0.05.
 *       ragged_matrix != 0 additionally sends references of unequal template lengths to dtw_ragged_kernel (same two-part products).
 * May be changed between calls (a template set serves every mode); rp_ctx_dtw_kernels reports what ran.  Returns 0, <0 on a bad value. */
enum { RP_ARITH_F32_MATRIX = 0, RP_ARITH_STRICT_F32 = 1, RP_ARITH_FAST_SPLIT = 2 };
int rp_ctx_set_arithmetic(rp_ctx *ctx, int arith, int ragged_matrix);
/* the current RP_ARITH_* (ragged_matrix, if not NULL, receives the flag) */
int rp_ctx_arithmetic(rp_ctx *ctx, int *ragged_matrix);
void rp_ctx_free(rp_ctx *ctx);
/* Run subsequent launches on an externally owned hipStream_t (e.g. the caller's
 * torch stream); NULL = the context's own stream. */
int rp_ctx_set_stream(rp_ctx *ctx, void *hip_stream);
int rp_ctx_synchronize(rp_ctx *ctx);
/* Diagnostics of the cosine distance (replaces nothing; src/mfcc/comparator.rs:28-48 is what it watches): the reference
 * divides by sqrt(dot_a * dot_b) in f32 and returns similarity 0 when that is 0.  The device kernels compare unit-length
 * vectors and hand every (window, templates) pair that met a squared norm outside 2^-60 .. 2^30 (frames) / 2^60 (template
 * rows) -- where the f32 product can underflow, lose bits or overflow -- to a reference-shaped kernel.  *pairs = the number
 * of pairs rescored that way by this context's DTW calls since it was made (waits for the context's stream); 0 for audio
 * in any ordinary range. */
int rp_ctx_dtw_ref_pairs(rp_ctx *ctx, uint64_t *pairs);
/* Diagnostics of the DTW dispatch (replaces nothing; src/mfcc/dtw.rs:56-105 is what every family computes): the kernel families this
 * context's DTW calls launched since the last call of this function, as a mask of RP_DTW_KERNEL_* (then cleared).  Tests and bench.py use
 * it to name the kernel a measurement belongs to. */
enum {
    RP_DTW_KERNEL_MFMA = 1,      /* dtw_mfma_kernel: chunks of 3..8 same-length templates, mfcc_size 5, cosines on the matrix cores */
    RP_DTW_KERNEL_MFMA_WIDE = 2, /* dtw_mfma_wide3_kernel (three bf16 parts) / dtw_mfma_wide_kernel (two f16 parts): mfcc_size 13 / 16 */
    RP_DTW_KERNEL_RAGGED = 4,    /* dtw_ragged_kernel: templates of unequal length on the matrix cores, mfcc_size 5 */
    RP_DTW_KERNEL_REGISTER = 8,  /* dtw_band_kernel / dtw_band2_kernel / dtw_band_wide_kernel: f32 vector arithmetic throughout */
    RP_DTW_KERNEL_GENERIC = 16,  /* dtw_generic_kernel */
    RP_DTW_KERNEL_SINGLE = 32,   /* dtw_single_kernel (a handful of windows of one stream) */
    RP_DTW_KERNEL_REF_ALL = 64,  /* dtw_ref_kernel over every window (a template row outside the norm range) */
    RP_DTW_KERNEL_MFMA_GROUP = 128, /* dtw_mfma_group_kernel: several chunks of one template length share a column's operand (same bits as MFMA) */
    /* the product arithmetic of the matrix-core launches among the above */
    RP_DTW_PRODUCTS_BF16X3 = 256,  /* three bf16 parts per operand: f32-grade (RP_ARITH_F32_MATRIX) */
    RP_DTW_PRODUCTS_F16X2 = 512,   /* two f16 parts per operand: 22 bits (RP_ARITH_FAST_SPLIT) */
    /* the builds of dtw_mfma_kernel launched among the above: waves per workgroup (same results either way) */
    RP_DTW_MFMA_WAVES_8 = 1024,    /* two waves per SIMD */
    RP_DTW_MFMA_WAVES_12 = 2048,   /* three waves per SIMD */
    RP_DTW_KERNEL_BANK = 4096,     /* dtw_bank_kernel: every stream against its own wakeword of a bank (rp_dtw_score_bank, rp_batch_detect_bank) */
    RP_DTW_KERNEL_BANK_STREAM = 8192, /* dtw_bank_stream_kernel: the same for the new windows of a live-stream batch (rp_stream_batch_new_bank) */
    RP_DTW_KERNEL_BANK_SETS = 16384,  /* dtw_set_kernel: every stream against its own SET of wakewords of a bank (rp_dtw_score_bank_sets, rp_batch_detect_bank_sets) */
    RP_DTW_KERNEL_BANK_SETS_STREAM = 32768, /* dtw_set_stream_kernel: the same for the new windows of a live-stream batch (rp_stream_batch_new_bank_sets) */
    RP_DTW_KERNEL_MIXED_SETS_STREAM = 65536 /* dtw_mixed_stream_kernel: the reference slots of a live-stream batch over mixed sets (rp_stream_batch_new_mixed_sets) */
};
int rp_ctx_dtw_kernels(rp_ctx *ctx);
/* Diagnostics of detect-only calls (replaces nothing): the first n floats of the [S * n_win][T] sample-template score workspace as the last
 * rp_batch_detect* of this context left it (waits for the context's stream; `out` is a HOST array whatever the context's flags say).
 * Fails when the context has made no such call or n exceeds what that call wrote.  An abandoned DTW holds 0 there.  Only defined after
 * UNGATED calls: the averaged-template gate (a detect-only call of a set with an averaged template and avg_threshold != 0) leaves the rows
 * it does not list as an earlier call wrote them.  Calls that hand their scores to a device array of the caller's, the several-wakeword
 * and model entry points and live-stream batches leave nothing to read here. */
int rp_ctx_last_window_scores(rp_ctx *ctx, float *out, size_t n);
/* Which build this library is (replaces nothing): the target architecture and the compiler flags it differs by from the
 * product's Makefile defaults -- "gfx950" for the product, "gfx950 +-DRP_..." for an experiment build (tools/ab.sh builds
 * those into rustpotter_amd/variants/, never over the product).  bench.py prints it on its JSON line. */
const char *rp_build_info(void);
/* Diagnostics of the wakeword-model forward (replaces nothing; src/wakewords/nn/wakeword_nn.rs:101-106 is what it computes): the
 * kernel(s) the last rp_mlp_forward_batch / rp_mlp_forward_windows / rp_batch_detect_model of this context ran and their operand format, e.g. "mlp_stream_kernel<f16x2 splits> +
 * mlp_mfma_kernel<f32> on listed rows".  The string belongs to the context and is valid until its next forward; "" before the first. */
const char *rp_ctx_last_mlp_kernel(rp_ctx *ctx);

/* Number of MFCC frames MfccExtractor::compute yields for a stream of n_samples fed
 * in 480-sample chunks from a fresh extractor: 3*floor(n/480) - 3
 * (src/mfcc/extractor.rs:60-79; the frame made of the first three shifts is never
 * emitted). */
size_t rp_mfcc_num_frames(size_t n_samples);

/* MfccExtractor::compute over whole streams, src/mfcc/extractor.rs:60-163.
 * pcm  [S][pcm_stride] f32 16 kHz mono (n_samples valid per stream)
 * mfcc [S][n_frames][K] f32, n_frames = rp_mfcc_num_frames(n_samples); K = mfcc_size
 * (set_out_size(K): K+1 filters/coefficients, coefficient 0 dropped). */
int rp_mfcc_batch(rp_ctx *ctx, const float *pcm, size_t S, size_t n_samples, size_t pcm_stride, int K, float *mfcc);

/* Same with the PCM in any of the reference's `Sample` formats (src/audio/audio_types.rs:59-137), host byte
 * order, decoded inside the kernel as `v as f32 / T::MAX as f32`: pcm [S][pcm_stride] of int8 / int16 /
 * int32 / float.  Halves (int16) the bytes the path reads from HBM. */
int rp_mfcc_batch_fmt(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                      int K, float *mfcc);

/* WakewordRef::new_from_sample_buffers (src/wakewords/comp/wakeword_ref_build.rs:9-41) followed by
 * WakewordSave::save_to_buffer (src/wakewords/wakeword_file.rs:22-26): builds a wakeword reference from
 * n 16 kHz wav buffers (PCM 8/16/32-bit or f32; first channel) -- MFCCs from the HIP kernel, whole-matrix
 * normalisation, DTW-aligned average template, rms level -- and returns it serialised as .rpw (CBOR) bytes
 * in *out_rpw (free with rp_buffer_free).  threshold / avg_threshold: NULL = None.  rms_from_files != 0
 * takes the MEDIAN sample level like new_from_sample_files (:80-81) instead of the maximum.
 * The bytes can be written to a file or handed to rp_add_wakeword_from_buffer. */
int rp_wakeword_ref_build(rp_ctx *ctx, const char *name, const float *threshold, const float *avg_threshold, size_t n,
                          const char *const *sample_names, const uint8_t *const *wav_buffers, const size_t *wav_lens,
                          uint16_t mfcc_size, int rms_from_files, uint8_t **out_rpw, size_t *out_len);
void rp_buffer_free(uint8_t *buffer);

/* MfccAverager::average (src/mfcc/averager.rs:5-37: DTW-aligned mean of templates, folded one after the other into the first) for W
 * wakewords at once, on the device, with the bits of the reference's f32 arithmetic.  counts [W] (>= 1): templates per wakeword; lens
 * [sum counts]: rows of each template, in FOLD order (the first of a wakeword is the origin); feats: all rows concatenated, [sum lens][K];
 * avg receives, concatenated, lens[first template of w] rows of K floats per wakeword (a wakeword of one template: that template).  HOST
 * arrays, like rp_templates_new.  Features must be finite. */
int rp_mfcc_average_batch(rp_ctx *ctx, size_t n_wakewords, int mfcc_size, const int32_t *counts, const int32_t *lens,
                          const float *feats, float *avg);

/* rp_wakeword_ref_build for W wakewords in one call: every wav parsed on the host, ONE MFCC launch over all samples, normalisation and
 * averaging on the device, one copy back.  names / thresholds / avg_thresholds / counts are [W] (NaN = None; either threshold array may be
 * NULL = all None); the samples of all wakewords follow each other in sample_names / wav_buffers / wav_lens [sum counts].  out_rpw /
 * out_lens [W]: one .rpw per wakeword -- the bytes rp_wakeword_ref_build gives for it -- each to be freed with rp_buffer_free.  A wakeword
 * the single call would refuse fails the whole call: the error is the single call's, prefixed "wakeword <index> (<name>): ", every
 * out_rpw[w] is NULL and nothing needs freeing. */
int rp_wakeword_ref_build_batch(rp_ctx *ctx, size_t n_wakewords, const char *const *names, const float *thresholds,
                                const float *avg_thresholds, const size_t *counts, const char *const *sample_names,
                                const uint8_t *const *wav_buffers, const size_t *wav_lens, uint16_t mfcc_size, int rms_from_files,
                                uint8_t **out_rpw, size_t *out_lens);

/* WakewordModelTrain::train_from_buffers (src/wakewords/nn/wakeword_model_train.rs:44-168) followed by
 * save_to_buffer: trains a wakeword model on the device from labelled wav samples and returns it as .rpw bytes.
 * A sample's label is the lower-cased text between '[' and ']' in its name ("none" without one).  Features =
 * the whole-file-normalised MFCC matrix of every sample (any sample rate, like rp_wakeword_ref_build), flattened,
 * zero-padded / truncated to the longest training sample; network shapes of ModelType Tiny / Small / Medium / Large
 * (src/wakewords/nn/wakeword_nn.rs:305-389); `epochs` full-batch steps of log_softmax + nll + SGD(learning_rate).
 * prev_model (NULL = none): an existing model .rpw to continue from -- its labels, type, mfcc_size and train_size
 * win over the options, as in the reference.  A fresh model's weights are drawn like candle_nn::linear does
 * (weights N(0, 2/fan_in), biases U(+-1/sqrt(fan_in))) from `seed` (the reference uses the thread RNG).
 * final_loss: the loss of the last epoch; test_accuracy: share of test samples whose arg-max label is right
 * (test_model :251-272); either may be NULL.  Errors as the reference: "No training data provided", "No test data
 * provided", "Your training data need to contain at least two labels", "Forbidden label '...'...". */
typedef enum { RP_MODEL_TINY = 0, RP_MODEL_SMALL = 1, RP_MODEL_MEDIUM = 2, RP_MODEL_LARGE = 3 } rp_model_type;
typedef struct {
    int m_type;            /* rp_model_type */
    float learning_rate;
    size_t epochs, test_epochs;   /* test_epochs only paces the reference's progress printing; unused */
    uint16_t mfcc_size;
    uint64_t seed;
} rp_train_options;
int rp_wakeword_model_train(rp_ctx *ctx, const rp_train_options *options, size_t n_train, const char *const *train_names,
                            const uint8_t *const *train_wavs, const size_t *train_lens, size_t n_test,
                            const char *const *test_names, const uint8_t *const *test_wavs, const size_t *test_lens,
                            const uint8_t *prev_model, size_t prev_model_len, uint8_t **out_rpw, size_t *out_len,
                            float *final_loss, float *test_accuracy);

/* rp_wakeword_model_train for W models in one call: enrol -> model bank (rp_model_bank_new_from_rpw) -> detect.  The epochs of all models
 * run side by side in one kernel, a workgroup per model, cut into launches of a bounded number of epochs (RP_TRAIN_EPOCHS_PER_LAUNCH, read
 * per call, replaces the default bound).  options holds what the models share (m_type, learning_rate, epochs, mfcc_size); the models may
 * differ in everything else: their samples, labels, window length and, through prev_models, type and mfcc_size.  train_counts /
 * test_counts [W]: samples per model; the samples of all models follow each other in train_names / train_wavs / train_lens [sum
 * train_counts] and test_names / test_wavs / test_lens [sum test_counts].  out_rpw / out_lens [W]: out_rpw[w] holds the bytes
 * rp_wakeword_model_train gives for model w's samples with options->seed replaced by seeds[w] (seeds NULL: options->seed + w) and
 * prev_models[w] (prev_models NULL or an entry NULL: none; prev_model_lens [W]); free each with rp_buffer_free.  final_loss /
 * test_accuracy: [W] or NULL.  A model the single call would refuse fails the whole call: the error is the single call's, prefixed
 * "model <index>: ", every out_rpw[w] is NULL and nothing needs freeing.  n_models == 0 succeeds and does nothing.  HOST arrays. */
int rp_wakeword_model_train_batch(rp_ctx *ctx, const rp_train_options *options, size_t n_models, const uint64_t *seeds,
                                  const size_t *train_counts, const char *const *train_names, const uint8_t *const *train_wavs,
                                  const size_t *train_lens, const size_t *test_counts, const char *const *test_names,
                                  const uint8_t *const *test_wavs, const size_t *test_lens, const uint8_t *const *prev_models,
                                  const size_t *prev_model_lens, uint8_t **out_rpw, size_t *out_lens, float *final_loss,
                                  float *test_accuracy);

/* The epochs alone (as rp_mfcc_average_batch is the averaging alone): W MLPs, each with its own shape and rows, `epochs` full-batch steps
 * of log_softmax + nll + SGD(learning_rate) with the arithmetic of rp_wakeword_model_train.  n_layers [W] (1..4); dims [W][5]: layer
 * widths, dims[w][0] the input, dims[w][n_layers[w]] the label count; n_rows [W] (>= 1); x: every model's rows concatenated ([n_rows][dims[0]]
 * each); labels likewise ([n_rows], 0 .. label count - 1); params in / out: per model, per layer, weight [out][in] then bias [out],
 * concatenated.  final_loss [W] or NULL: the loss of the last epoch (NaN for 0 epochs).  A model that cannot be trained fails the whole
 * call ("model <index>: ...") and leaves params as they were.  HOST arrays. */
int rp_mlp_train_batch(rp_ctx *ctx, size_t n_models, const int32_t *n_layers, const int32_t *dims, const int32_t *n_rows,
                       const float *x, const int32_t *labels, float *params, float learning_rate, size_t epochs, float *final_loss);

/* What the context's last rp_wakeword_model_train_batch / rp_mlp_train_batch call spent (tools/bench_train_batch.py): feature_ms, the
 * host's time in the feature stage (wav decoding, resampling and MFCCs, one sample after the other; 0 for rp_mlp_train_batch);
 * launches, the kernel launches of its epochs; longest_launch_ms, the longest of them, timed with hipEvents -- 0 unless
 * rp_ctx_timing_enable was on during the call.  Any of the three may be NULL. */
int rp_train_batch_last_profile(rp_ctx *ctx, double *feature_ms, double *longest_launch_ms, int *launches);

/* The audio front-end of Rustpotter::process_audio for whole streams (src/detector.rs:358-371): sample
 * decode, GainNormalizerFilter (src/audio/gain_normalizer_filter.rs:14-55: per 480-sample chunk, gain =
 * round(10*sqrt(ref)/sqrt(mean of the last `window_size` chunk RMS values))/10, clamped, samples clamped to
 * +-1) and BandPassFilter (src/audio/band_pass_filter.rs:19-55: biquad with state carried along the
 * stream).  Neither filter depends on detections (reset() keeps them), so the result is what the
 * detector would have fed its MFCC extractor.  rms_level_ref: what on_wakeword_change sets (the largest
 * wakeword rms_level) -- ignored when filters->gain_normalizer.has_gain_ref; window_size: max_mfcc_frames / 3
 * (src/detector.rs:337).  pcm_out [S][out_stride] f32; rms / gains [S][n_samples/480] (either may be NULL):
 * get_rms_level() and get_gain() of every chunk. */
int rp_frontend_batch(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                      const rp_filters_config *filters, float rms_level_ref, size_t window_size, float *pcm_out,
                      size_t out_stride, float *rms, float *gains);

/* A wakeword reference resident on the device: T templates [len_t][K] (already
 * mean-normalised, as stored in a .rpw: src/wakewords/wakeword_ref.rs:12-20) given
 * as HOST arrays; avg may be NULL. */
int rp_templates_new(rp_ctx *ctx, int T, int K, const int *lens, const float *feats, int avg_len, const float *avg,
                     rp_templates **out);
void rp_templates_free(rp_templates *t);
int rp_templates_max_len(const rp_templates *t);

/* WakewordComparator::run_detection scoring for every window start of every stream,
 * src/wakewords/comp/wakeword_comp.rs:22-37,77-139 + src/mfcc/comparator.rs +
 * src/mfcc/dtw.rs:56-105 + src/mfcc/normalizer.rs.  n_win = n_frames - max_len + 1.
 * scores [S][n_win][T]; avg [S][n_win] (NULL or ignored when the template set has no
 * avg template / with_avg == 0); agg [S][n_win] = score_mode aggregate.  band_size 0 is
 * legal as in the reference (u16): no cell lies in the band and every score is 0.  The aggregate takes at most 256 sample
 * templates: with agg != NULL (and in every detect call) a template set of more is an error that names the limit. */
int rp_dtw_score_batch(rp_ctx *ctx, const float *mfcc, size_t S, size_t n_frames, const rp_templates *t,
                       float score_ref, int band_size, rp_score_mode score_mode, int with_avg,
                       float *scores, float *avg, float *agg);

/* One detection found by rp_detect_scan */
typedef struct {
    int32_t stream;
    int32_t frame;       /* index of the MFCC frame whose processing emitted the detection */
    int32_t window;      /* window start (frame index) of the best partial = row of `scores` */
    int32_t counter;     /* RustpotterDetection::counter */
    float avg_score;
    float score;
} rp_batch_detection;

/* Rustpotter::process_new_mfccs / run_detection / reset state machine,
 * src/detector.rs:290-302,377-454, run over precomputed window scores.  With config->vad_mode set,
 * the VadDetector gate (src/mfcc/vad.rs:11-36, :379-383) is evaluated per stream from `mfcc`
 * ([S][n_frames][K], required then; may be NULL otherwise).
 * det [S][max_det] (device or host per ctx flag), n_det [S] (may exceed max_det: only the first max_det detections of a
 * stream are stored; slots behind a stream's detections are zero).  agg / avg are [S][n_win] with n_win = n_frames - max_len + 1
 * (0 when n_frames < max_len); max_len < 1 and max_det < 0 are errors. */
int rp_detect_scan(rp_ctx *ctx, const float *agg, const float *avg, size_t S, size_t n_frames, int max_len,
                   const rp_detector_config *config, int avg_enabled, const float *mfcc, int K,
                   rp_batch_detection *det, int32_t *n_det, int max_det);

/* The whole path for S independent streams in one call = S x (Rustpotter::new + add_wakeword +
 * process_samples over the stream in 480-sample chunks), src/detector.rs:347-454: MFCC -> window
 * scores -> score_mode aggregate -> detection state machine; intermediate arrays live in buffers
 * owned by the context (grown on demand, reused across calls).  pcm [S][pcm_stride] f32 16 kHz mono;
 * det [S][max_det], n_det [S] as in rp_detect_scan.  Optional outputs (NULL to skip): scores
 * [S][n_win][T] and agg [S][n_win] with n_win = rp_mfcc_num_frames(n_samples) - max_len + 1.
 * The wakeword's own threshold / avg_threshold overrides (Option<f32> in the .rpw) are passed in
 * `config` by the caller; avg gate as in WakewordComparator::run_detection :83-93: with an averaged template and
 * avg_threshold != 0, windows whose avg_score is below the threshold are NOT compared with the sample templates
 * (one DTW instead of T+1) unless `scores` / `agg` are requested -- those arrays hold every window -- or the
 * context has RP_CTX_FULL_SCORES; the detections are the same on either path.  A call that asks for neither array is
 * "detect-only": in ScoreMode::Max it may also stop DTWs whose running cost already rules out a score above
 * `threshold` (cell costs are >= 0, so the cost can only grow) -- only where a whole wave of 64 windows is past that bound,
 * so every window that can fire keeps exact scores and the detections do not change. */
int rp_batch_detect(rp_ctx *ctx, const float *pcm, size_t S, size_t n_samples, size_t pcm_stride, const rp_templates *t,
                    const rp_detector_config *config, rp_batch_detection *det, int32_t *n_det, int max_det,
                    float *scores, float *agg);

/* rp_batch_detect with the PCM in any sample format (see rp_mfcc_batch_fmt). */
int rp_batch_detect_fmt(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                        const rp_templates *t, const rp_detector_config *config, rp_batch_detection *det, int32_t *n_det,
                        int max_det, float *scores, float *agg);

/* rp_batch_detect_fmt for streams that live in HOST memory, pipelined (the serving shape of `process_samples` over many
 * streams, src/detector.rs:234-254: the audio arrives in host buffers): the S streams are taken in blocks of `block_streams`
 * (0 = 8 192); block k+1's host-to-device copy runs on the context's copy stream while block k's kernels run on its launch
 * stream, two device blocks are cycled, the detections of every block are copied back as it finishes.  pcm [S][pcm_stride],
 * det [S][max_det] and n_det [S] are HOST arrays whatever the context's RP_CTX_HOST_POINTERS flag says; detection records carry
 * global stream ids.  The copies overlap the kernels when the host memory is page-locked (hipHostMalloc / hipHostRegister by the
 * caller: the link then runs at its rate and binds -- 862 B per scoring for f32, half for i16); pageable memory works, copy by
 * copy.  Device memory needed: two blocks of PCM + one block's intermediates, so S may exceed what fits in HBM at once.
 * seconds (NULL to skip): wall time of the call. */
int rp_batch_detect_ingest(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                           const rp_templates *t, const rp_detector_config *config, rp_batch_detection *det, int32_t *n_det,
                           int max_det, size_t block_streams, double *seconds);

/* Multi-GPU form of rp_batch_detect_fmt: independent streams shard across the GPUs of a node, nothing is
 * exchanged but the final per-stream results.  The caller owns one context per device (rp_ctx_new(device g)) with the
 * wakeword replicated on each (rp_templates_new on every context; <= 128 KB).  Shard g = S[g] streams whose PCM
 * pcm[g] lives on ctxs[g]'s device (or in host memory if the contexts have RP_CTX_HOST_POINTERS); global stream ids are
 * assigned in shard order (shard g holds streams sum(S[0..g)) .. ).  One host thread per shard drives its device and
 * stream -- the reference's `Rustpotter: Send`, one detector per thread -- and every shard's detections are gathered
 * into ONE block: det [sum S][max_det] / n_det [sum S], `stream` fields holding global ids, in host memory
 * (RP_CTX_HOST_POINTERS) or on ctxs[0]'s device (peer copies over xGMI).  Returns when the gathered block is complete.
 * Same detections as one rp_batch_detect_fmt call over the concatenated streams. */
int rp_batch_detect_sharded(rp_ctx *const *ctxs, const rp_templates *const *t, int n_shards, const void *const *pcm,
                            rp_sample_format fmt, const size_t *S, size_t n_samples, size_t pcm_stride,
                            const rp_detector_config *config, rp_batch_detection *det, int32_t *n_det, int max_det);
/* How the calling thread's last rp_batch_detect_sharded gathered the shards' results (replaces nothing; SURVEY 8e's final gather):
 * per shard whether its device writes into the gathering device directly (peer access over xGMI) or the runtime stages the copy.
 * Valid until the thread's next sharded call; "" before the first. */
const char *rp_sharded_gather_info(void);

/* rp_batch_detect for a detector that holds SEVERAL wakewords (run_wakeword_detectors, src/detector.rs:433-447: every
 * wakeword whose own thresholds pass proposes a detection for the frame, the best score wins; max_mfcc_frames is the
 * longest template over all wakewords and each wakeword scores the oldest frames of that window,
 * wakeword_comp.rs:22-27).  t [n_wakewords] (1..8, all with the same mfcc_size, else the reference's "Usage of
 * wakewords with different mfcc size is not supported, ignoring wakeword"); thresholds / avg_thresholds
 * [n_wakewords]: the wakeword's own Option<f32> overrides, NaN = the value in `config` (either array may be NULL).
 * det_wakeword [S][max_det] (NULL to skip): index of the wakeword a detection belongs to. */
int rp_batch_detect_multi(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                          size_t n_wakewords, const rp_templates *const *t, const rp_detector_config *config,
                          const float *thresholds, const float *avg_thresholds, rp_batch_detection *det,
                          int32_t *det_wakeword, int32_t *n_det, int max_det);

/* Personal wakewords: a wakeword BANK -- W wakeword references uploaded once -- and calls in which stream s carries its own wakeword
 * stream_wakeword[s].  The batched form of one `Rustpotter` per thread, each holding one wakeword (src/detector.rs:304-346): enrol
 * (rp_wakeword_ref_build_batch) -> bank -> detect.  A bank borrows `ctx`, which must outlive it, and is used with that context only.
 * Arithmetic: bank calls always score with f32 vector FMAs, the arithmetic of RP_ARITH_STRICT_F32, whatever rp_ctx_set_arithmetic says
 * (the setting is neither read nor changed); a stream gets the bits rp_batch_detect / rp_dtw_score_batch give it under RP_ARITH_STRICT_F32
 * with its wakeword as rp_templates.  (One exception, in the last bits only: a window whose only frame outside the norm range of the fast
 * cosine lies within band_size - 2 frames BEHIND its end is rescored with the reference-shaped cosine by a bank call, and not by an
 * rp_dtw_score_batch call of one stream with at most 8 windows, RP_DTW_KERNEL_SINGLE, which never loads those frames.  Both are within
 * the parity bar.)  rp_ctx_dtw_kernels reports RP_DTW_KERNEL_BANK.
 * Limits (refused with an error that names them): at most RP_WAKEWORD_BANK_MAX_TEMPLATES sample templates per wakeword; mfcc_size 5, 13 or
 * 16 with band_size 3..6 (the pairs the register kernels are built for), or band_size 0 (every score 0, as everywhere); an averaged
 * template no longer than the wakeword's longest sample template (src/mfcc/averager.rs:5-37 folds into the first sample: never a longer one); a
 * longest sample template of at most 7546 / 2859 / 2170 frames at mfcc_size 5 / 13 / 16 (a tile's frames for it fill the 160 KB of LDS;
 * other sizes: the limit the error names).  Wakeword models cannot be part of a wakeword bank: they have a bank of their own, rp_model_bank.
 * An empty bank (n_wakewords == 0) is a Rustpotter without wakewords: calls succeed for any band_size with every index -1, report no
 * detection and write zero rows. */
enum { RP_WAKEWORD_BANK_MAX_TEMPLATES = 32 };
typedef struct rp_wakeword_bank rp_wakeword_bank;
/* WakewordRef (src/wakewords/wakeword_ref.rs:12-20) x n_wakewords from HOST arrays in the flat layout of rp_mfcc_average_batch: counts
 * [W] (1..RP_WAKEWORD_BANK_MAX_TEMPLATES) sample templates per wakeword, lens [sum counts] (>= 1) rows of each, feats [sum lens][mfcc_size]
 * (finite; already mean-normalised, as stored in a .rpw); avg_lens [W] rows of each wakeword's averaged template, 0 = none, and avg_feats
 * [sum avg_lens][mfcc_size] (both may be NULL: no averaged templates); thresholds / avg_thresholds [W]: the wakeword's own Option<f32>,
 * NaN = None = the value of the call's config applies, as in rp_batch_detect_multi (either array may be NULL).  A wakeword that is refused
 * fails the call with "wakeword <index>: <reason>". */
int rp_wakeword_bank_new(rp_ctx *ctx, size_t n_wakewords, int mfcc_size, const int32_t *counts, const int32_t *lens, const float *feats,
                         const int32_t *avg_lens, const float *avg_feats, const float *thresholds, const float *avg_thresholds,
                         rp_wakeword_bank **out);
/* The same from .rpw bytes (WakewordLoad::load_from_buffer, src/wakewords/wakeword_file.rs:38; src/detector.rs:152-176) -- what
 * rp_wakeword_ref_build_batch returns goes straight in.  Each wakeword keeps its own threshold / avg_threshold Options.  A wakeword model,
 * a file the reader refuses or a wakeword whose mfcc_size differs from the first one's fails the whole call: "wakeword <index>: <reason>"
 * (src/detector.rs:310-320: "Usage of wakewords with different mfcc size is not supported, ignoring wakeword"). */
int rp_wakeword_bank_new_from_rpw(rp_ctx *ctx, size_t n_wakewords, const uint8_t *const *rpw_buffers, const size_t *rpw_lens,
                                  rp_wakeword_bank **out);
void rp_wakeword_bank_free(rp_wakeword_bank *bank);
/* WakewordComparator::get_mfcc_frame_size (src/wakewords/comp/wakeword_comp.rs:69-75): the longest sample template of that wakeword = its
 * window length; wakeword < 0: the longest in the bank (0 for an empty bank).  -1 for a NULL bank or an index outside the bank. */
int rp_wakeword_bank_max_len(const rp_wakeword_bank *bank, long long wakeword);
/* WakewordRef::rms_level of every wakeword (src/wakewords/wakeword_ref.rs:12-20), the reference level the gain normaliser of a detector
 * that holds that wakeword works towards (on_wakeword_change, src/detector.rs:328-338): kept from the .rpw files by
 * rp_wakeword_bank_new_from_rpw, NaN for every wakeword of a bank made by rp_wakeword_bank_new (NaN = no reference level: the gain stays 1,
 * gain_normalizer_filter.rs:15).  rms_levels: a HOST array [n_wakewords], NaN allowed, whatever the pointer flag of the context; the write
 * is ordered on the context's stream and holds from the next call that uses the bank (rp_frontend_batch_bank, a live-stream batch with
 * rp_stream_batch_set_filters_bank). */
int rp_wakeword_bank_set_rms_levels(rp_wakeword_bank *bank, const float *rms_levels);
/* ... of one wakeword as last set; NaN for a NULL bank or an index outside the bank. */
float rp_wakeword_bank_rms_level(const rp_wakeword_bank *bank, long long wakeword);
/* ---- A bank that changes: enrol and replace wakewords, also under live-stream batches.
 * rp_wakeword_bank_put / _put_from_rpw / _enrol write the wakewords first .. first + n - 1.  first <= rp_wakeword_bank_size is required (a bank
 * has no holes): indices below the size are REPLACED, indices at or above it extend the bank; n == 0 succeeds and changes nothing.  Every
 * limit and wording of rp_wakeword_bank_new / _new_from_rpw applies per wakeword ("wakeword <index>: <reason>", <index> = the bank index
 * first + i): 1..RP_WAKEWORD_BANK_MAX_TEMPLATES templates, finite features, an averaged template no longer than the window, the length limit of
 * the device kernels, no wakeword models, one mfcc_size (the bank's; a .rpw of another is refused with the reference's "different mfcc size"
 * text.  Only an empty bank without a reserved length and without a stream batch takes the mfcc_size of the first file put into it).  A call
 * that is refused or fails leaves the bank exactly as it was: size, longest window, rms levels, every score.
 * Storage: the bank's device arrays are pools.  New templates are appended, a replaced wakeword's old ones stay behind as garbage, and a full
 * pool is replaced by one of at least twice the size into which only the live templates move (on the device) -- growth is the compaction.
 * Ordering: every update is enqueued on the context's stream behind whatever still reads the bank, and the call returns after it has
 * completed (as rp_wakeword_bank_set_rms_levels).  The next call that uses the bank sees the new contents, the next rp_stream_batch_process
 * of a live batch over it included; nothing in flight ever sees a half-written wakeword.
 * Live-stream batches: a batch sizes every stream's MFCC history and gain ring once, so the bank must never come to hold a window longer than
 * a live batch has room for.  rp_wakeword_bank_reserve(max_len) declares the longest window the bank will ever hold: put / enrol refuse a
 * longer one, and rp_stream_batch_new_bank keeps room for max(reserved, longest now, 1) frames.  Without a reserved length, while a batch
 * over the bank exists, a wakeword longer than the current longest is refused (the error says to call rp_wakeword_bank_reserve before
 * creating the batch); without either, any admissible length goes.  The bank counts its batches (a batch is freed before its bank).
 * The bank does not touch batches: a stream that holds an index while that index is replaced scores the new templates from the next call on,
 * with the detector state it has (and the gain normaliser of rp_stream_batch_set_filters_bank reads the new level and window size, as
 * it reads them at the start of every call).  For the reference's remove_wakeword + add_wakeword, call rp_stream_batch_set_wakewords for
 * those streams: it resets them as it always does.  Removing a wakeword is not offered: disconnect its streams; the next put reuses the slot. */
/* max_len > 0: no wakeword's window may become longer.  At least the current longest and within the length limit of the device kernels for the
 * bank's mfcc_size; it can change only while no stream batch over the bank exists.  max_len == 0 leaves it as it is.  n_wakewords / n_rows
 * pre-size the pools for that many wakewords / template rows (averaged templates included) in all; 0 leaves them; hints, never limits.
 * A reserved bank of n_wakewords == 0 is the natural starting state of a service: a batch over it takes the bank's declared mfcc_size, and
 * its (mfcc_size, band_size) pair is checked although it is empty. */
int rp_wakeword_bank_reserve(rp_wakeword_bank *bank, int max_len, size_t n_wakewords, size_t n_rows);
/* wakewords in the bank; -1 for a NULL bank */
int rp_wakeword_bank_size(const rp_wakeword_bank *bank);
/* the reserved length, 0 = none; -1 for a NULL bank */
int rp_wakeword_bank_reserved_len(const rp_wakeword_bank *bank);
/* how often the template pools have been replaced by larger ones so far (tests and capacity planning); -1 for a NULL bank */
int rp_wakeword_bank_pool_growths(const rp_wakeword_bank *bank);
/* HOST arrays in the flat layout of rp_wakeword_bank_new for the n wakewords, whatever the pointer flag of the context; rms_levels [n]: each
 * wakeword's reference level (NULL = NaN for all, as rp_wakeword_bank_new leaves them).  The rows are prepared on the device
 * (bank_put_kernel) with the bits rp_wakeword_bank_new gives them. */
int rp_wakeword_bank_put(rp_wakeword_bank *bank, size_t first, size_t n, const int32_t *counts, const int32_t *lens, const float *feats,
                         const int32_t *avg_lens, const float *avg_feats, const float *thresholds, const float *avg_thresholds,
                         const float *rms_levels);
/* The same from .rpw bytes, as rp_wakeword_bank_new_from_rpw: each wakeword keeps its file's thresholds and rms_level. */
int rp_wakeword_bank_put_from_rpw(rp_wakeword_bank *bank, size_t first, size_t n, const uint8_t *const *rpw_buffers, const size_t *rpw_lens);
/* Enrolment straight into bank slots: the arguments of rp_wakeword_ref_build_batch (mfcc_size is the bank's; thresholds NaN = None), the same
 * stages up to the averaged template, and from there the templates go from the enrolment workspace into the bank on the device -- no feature
 * round trip.  Each wakeword's rms_level is what rp_wakeword_bank_new_from_rpw would take from its file.  out_rpw / out_lens [n] may both be
 * NULL; given, they receive exactly rp_wakeword_ref_build_batch's bytes (free each with rp_buffer_free), and on failure every entry is NULL. */
int rp_wakeword_bank_enrol(rp_wakeword_bank *bank, size_t first, size_t n, const char *const *names, const float *thresholds,
                           const float *avg_thresholds, const size_t *counts, const char *const *sample_names,
                           const uint8_t *const *wav_buffers, const size_t *wav_lens, int rms_from_files, uint8_t **out_rpw, size_t *out_lens);
/* rp_frontend_batch with every stream's OWN gain-normaliser parameters, what goes in front of rp_batch_detect_bank: stream s works towards
 * rms_level_ref = the rms_level of bank[stream_wakeword[s]] (filters->gain_normalizer.gain_ref for every stream when has_gain_ref) over a
 * window of max(max_len(s) / 3, 1) chunk levels (src/detector.rs:337).  stream_wakeword[s] == -1 is a detector without wakewords, whose
 * process_audio returns before the filters (src/detector.rs:348-350): its gain is 1 for every chunk and its samples pass the gain stage
 * unchanged; the band-pass filter, when enabled, runs on such a stream like on any other and its chunk levels are reported -- what a
 * live-stream batch over a bank does.  stream_wakeword [S] int32, checked as in rp_dtw_score_bank: with RP_CTX_HOST_POINTERS an index
 * outside [-1, n_wakewords) is an error found before anything is launched or written; with device arrays the kernels treat it as -1.
 * Everything else as rp_frontend_batch. */
int rp_frontend_batch_bank(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                           const rp_filters_config *filters, const rp_wakeword_bank *bank, const int32_t *stream_wakeword,
                           float *pcm_out, size_t out_stride, float *rms, float *gains);
/* rp_dtw_score_batch for a bank (src/wakewords/comp/wakeword_comp.rs:22-37,77-139 per stream with its own wakeword): mfcc [S][n_frames][K],
 * stream_wakeword [S] int32 (-1: the stream has no wakeword).  agg and avg (avg may be NULL) are [S][win_pitch]: row s holds
 * n_win_s = n_frames - max_len(wakeword of s) + 1 values (the score_mode aggregate; the averaged template's score when with_avg != 0 and
 * the wakeword has one, else 0) and zeros behind them up to win_pitch; a stream without a wakeword or shorter than its window has an
 * all-zero row.  win_pitch smaller than the largest n_win_s of the call is an error.  With RP_CTX_HOST_POINTERS an index outside
 * [-1, n_wakewords) is an error, found before anything is launched; with device arrays the kernels treat such an index as -1 and win_pitch
 * must hold the largest window count any wakeword of the bank gives. */
int rp_dtw_score_bank(rp_ctx *ctx, const float *mfcc, size_t S, size_t n_frames, const rp_wakeword_bank *bank, const int32_t *stream_wakeword,
                      float score_ref, int band_size, rp_score_mode score_mode, int with_avg, float *avg, float *agg, size_t win_pitch);
/* rp_batch_detect for a bank: stream s = Rustpotter::new(config) + add_wakeword(bank[stream_wakeword[s]]) + process_samples over the
 * stream (src/detector.rs:304-346,347-454): max_mfcc_frames is that wakeword's longest sample template, every template scores the oldest
 * `len` frames of the window (wakeword_comp.rs:22-27), the wakeword's own thresholds override config's, the averaged-template test runs
 * only when the wakeword has an averaged template and its effective avg_threshold != 0 (:83-93), the countdown is max_len / 2; reset and
 * VAD as in rp_batch_detect.  stream_wakeword[s] == -1: a Rustpotter without wakewords -- n_det[s] = 0 (indices as in rp_dtw_score_bank).
 * det [S][max_det], n_det [S] as in rp_detect_scan.  agg / avg (either may be NULL) [S][win_pitch] as in rp_dtw_score_bank, with the
 * semantics of rp_batch_detect's agg: when either is requested, or the context has RP_CTX_FULL_SCORES, every window is fully scored;
 * otherwise (detect-only) a wave of 64 windows none of which passes the averaged-template gate skips the sample templates -- the
 * detections are the same either way.  win_pitch is only read when agg or avg is requested. */
int rp_batch_detect_bank(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                         const rp_wakeword_bank *bank, const int32_t *stream_wakeword, const rp_detector_config *config,
                         rp_batch_detection *det, int32_t *n_det, int max_det, float *agg, float *avg, size_t win_pitch);

/* Wakeword SETS: several personal wakewords per stream over a bank.  stream_wakewords [S][set_size] (set_size 1..RP_WAKEWORD_SET_MAX) holds
 * up to set_size bank indices per stream; -1 marks an empty slot, anywhere in the row, and a row of all -1 is a detector without wakewords.
 * Stream s behaves as Rustpotter::new(config) followed by add_wakeword(bank[i]) for its live slots in slot order, then process_samples
 * (add_wakeword, on_wakeword_change, run_wakeword_detectors: src/detector.rs:304-346,433-447): max_mfcc_frames = Lmax(s), the longest
 * window over the stream's live slots; every wakeword scores the OLDEST len frames of that window (wakeword_comp.rs:22-27) with its own
 * thresholds over the config's, the averaged-template test only where it has an averaged template and its effective avg_threshold != 0
 * (wakeword_comp.rs:85); the best passing score wins, of equal scores the first slot; the countdown is Lmax(s) / 2; a detection reports
 * window = frame - Lmax(s) + 1 and the BANK index of the winner.  Duplicate indices in a row are allowed and change nothing.  Arithmetic
 * and limits are those of the bank calls above: f32 vector FMAs whatever rp_ctx_set_arithmetic says, mfcc_size 5 / 13 / 16 with band_size
 * 3..6, or band_size 0 (every score 0, no detection); empty banks and all -1 rows succeed and report nothing.  With RP_CTX_HOST_POINTERS an
 * index outside [-1, n_wakewords) is an error that names stream and slot, found before anything is allocated or launched; with device arrays
 * the kernels treat such an index as -1 (and win_pitch must then hold the window count of the bank's shortest wakeword).
 * rp_ctx_dtw_kernels reports RP_DTW_KERNEL_BANK_SETS. */
enum { RP_WAKEWORD_SET_MAX = 8 };
/* rp_dtw_score_bank over sets: agg and avg (avg may be NULL; scored with with_avg where a wakeword has an averaged template) are
 * [S][set_size][win_pitch].  Row (s, j) holds n_win_s = n_frames - Lmax(s) + 1 values, the scores of wakeword set[s][j] for the windows
 * that start at frames 0 .. n_win_s - 1 -- the first n_win_s values of rp_dtw_score_bank's row for that wakeword, bit for bit -- and zeros
 * behind them; an empty slot has an all-zero row.  A stream shorter than Lmax(s) has all-zero rows in every slot although a shorter
 * wakeword of its set would fit: the reference's window never fills (src/detector.rs:377-392).  win_pitch below the largest n_win_s of
 * the call is refused. */
int rp_dtw_score_bank_sets(rp_ctx *ctx, const float *mfcc, size_t S, size_t n_frames, const rp_wakeword_bank *bank,
                           const int32_t *stream_wakewords, int set_size, float score_ref, int band_size, rp_score_mode score_mode, int with_avg,
                           float *avg, float *agg, size_t win_pitch);
/* rp_batch_detect_bank over sets (run_wakeword_detectors, src/detector.rs:433-447, per stream): det_wakeword [S][max_det] (NULL to skip)
 * is the bank index of the wakeword each detection belongs to.  agg / avg (either may be NULL) are the per-slot rows
 * [S][set_size][win_pitch] laid out as in rp_dtw_score_bank_sets, avg scored where a wakeword's test runs.  Detection itself never
 * materialises them: the kernel folds every window's proposal (best passing score, its avg score, its bank index) into three rows
 * [S][n_win].  Detect-only calls (agg == avg == NULL, no RP_CTX_FULL_SCORES) may leave windows below their avg_threshold uncompared, as
 * rp_batch_detect_bank; the detections are the same either way.  VAD and the reset after a detection as everywhere. */
int rp_batch_detect_bank_sets(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                              const rp_wakeword_bank *bank, const int32_t *stream_wakewords, int set_size, const rp_detector_config *config,
                              rp_batch_detection *det, int32_t *det_wakeword, int32_t *n_det, int max_det, float *agg, float *avg,
                              size_t win_pitch);

/* Sample-rate conversion in front of the path: AudioEncoder::new / reencode_to_mono_with_sample_rate
 * (src/audio/encoder.rs:41-60,63-83), i.e. rubato's FftFixedInOut<f32>::new(sample_rate, 16000, 480, 1) and one
 * process_into_buffer per input frame.  rp_resampler_frame_lengths gives AudioEncoder's
 * get_input_frame_length() (per channel) and the number of 16 kHz samples one input frame yields (48 kHz:
 * 1440 -> 480).  Returns 0, or -1 for a rate the resampler cannot be built for ("Unsupported sample rate,
 * unable to initialize the resampler", encoder.rs:78). */
int rp_resampler_frame_lengths(size_t sample_rate, size_t *in_len, size_t *out_len);
/* Whole streams: pcm [S][pcm_stride] in `fmt`, `channels` interleaved channels (the first one is used,
 * encoder.rs:42-48), n_samples frames per stream at `sample_rate`; chunks_exact(in_len) frames are converted
 * (a shorter tail is dropped, src/mfcc/wav_file_extractor.rs:83-96), the stream starts from silence.
 * out [S][out_stride] receives (n_samples / in_len) * out_len f32 samples at 16 kHz per stream. */
int rp_resample_batch(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, int channels, size_t sample_rate, size_t S,
                      size_t n_samples, size_t pcm_stride, float *out, size_t out_stride);

/* Live streams: S detectors that each receive n_chunks 30 ms chunks per call -- the batched form of
 * calling Rustpotter::process_samples (src/detector.rs:347-376) once per chunk on S independent
 * instances that share one wakeword and one DetectorConfig.  Everything the reference keeps between
 * calls stays on the device: the previous chunk (MfccExtractor's sample history, src/mfcc/extractor.rs),
 * the last max_len-1 MFCC frames (Rustpotter::audio_mfcc_window), the partial detection / countdown
 * (src/detector.rs:62-79) and the VadDetector window.  Frames are numbered as in rp_batch_detect
 * (frame f is the f-th MFCC frame since the batch was created), so feeding a stream in pieces gives
 * the detections of rp_batch_detect over the concatenation. */
/* Lifetime: a stream batch borrows `ctx` and `t` -- both must outlive it (free the batch first).  A call that fails
 * (-1) leaves the batch unusable: part of its device state may already have advanced, so every later
 * rp_stream_batch_process on it fails with "stream batch is in a failed state"; free it and create a new one. */
typedef struct rp_stream_batch rp_stream_batch;
int rp_stream_batch_new(rp_ctx *ctx, const rp_templates *t, const rp_detector_config *config, size_t S,
                        size_t max_chunks_per_call, rp_stream_batch **out);
void rp_stream_batch_free(rp_stream_batch *b);
/* pcm [S][pcm_stride] holds n_chunks * rp_stream_batch_samples_per_chunk() new samples per stream (480 per chunk by
 * default; 1 <= n_chunks <= max_chunks_per_call).
 * det [S][max_det], n_det [S]: detections emitted during these chunks (n_det may exceed max_det; only
 * the first max_det are stored).  agg (NULL to skip) [S][3*n_chunks]: aggregate score of the window
 * ending at each new frame (garbage for windows that reach before frame 0).  Without `agg` (and without
 * RP_CTX_FULL_SCORES) windows below avg_threshold are not compared with the sample templates, as in rp_batch_detect. */
int rp_stream_batch_process(rp_stream_batch *b, const void *pcm, rp_sample_format fmt, size_t n_chunks, size_t pcm_stride,
                            rp_batch_detection *det, int32_t *n_det, int max_det, float *agg);
/* The AudioFmt of the streams (RustpotterConfig.fmt: sample_rate, channels; src/config.rs:10-29), to be set before
 * the first rp_stream_batch_process -- default 16 kHz mono.  Input that is not 16 kHz is converted per call
 * exactly as one Rustpotter per stream would (the first channel of every frame, rubato-style resampling with the
 * previous input frame of every stream kept on the device; the resampler is not touched by resets).  A chunk is
 * then rp_stream_batch_samples_per_chunk() samples (= get_samples_per_frame(): 1 440 for 48 kHz mono).  For the
 * 11.025 / 22.05 kHz family a chunk is a 40 ms frame (640 encoded samples): a stream then gains four MFCC frames per
 * chunk (agg has 4 * n_chunks columns) and a detection drops the rest of its 40 ms frame, as in the reference. */
int rp_stream_batch_set_input(rp_stream_batch *b, size_t sample_rate, int channels);
size_t rp_stream_batch_samples_per_chunk(const rp_stream_batch *b);
/* Rustpotter::reset (src/detector.rs:290-302) of one stream, or of all when stream < 0. */
int rp_stream_batch_reset(rp_stream_batch *b, long long stream);
/* chunks consumed so far (per stream) */
size_t rp_stream_batch_chunks_seen(const rp_stream_batch *b);
/* RustpotterConfig.filters for the streams of a batch (src/detector.rs:358-371).  To be called before the first
 * rp_stream_batch_process (like rp_stream_batch_set_input; either order of the two).  rms_level_ref: what
 * on_wakeword_change would set (src/detector.rs:328-338: the largest rms_level of the detector's wakewords; NaN =
 * none, the gain then stays 1) -- ignored when filters->gain_normalizer.has_gain_ref.  The window of the gain
 * normaliser is max_mfcc_frames / 3 (0 -> 1) with max_mfcc_frames the batch's longest wakeword, as :337.
 * Per encoded 480-sample chunk and stream, as process_audio does: RMS level of the unfiltered chunk, gain normaliser,
 * band-pass, then MFCC.  The state of both filters (the window of chunk levels, the biquad's last two inputs and
 * outputs) lives on the device per stream for the life of the batch and is NOT touched by rp_stream_batch_reset
 * (Rustpotter::reset leaves the filters alone).  With both filters disabled the batch runs as if this had not been
 * called, except that rp_stream_batch_levels reports the chunk levels (gains of 1).  Not available together with the
 * 40 ms input frames of 11.025 / 22.05 kHz input: whichever of this and rp_stream_batch_set_input comes second fails. */
int rp_stream_batch_set_filters(rp_stream_batch *b, const rp_filters_config *filters, float rms_level_ref);
/* get_rms_level() / get_gain() of every chunk of the LAST rp_stream_batch_process[_multi] call of a batch that has had
 * rp_stream_batch_set_filters: rms, gains [S][n_chunks of that call] (either may be NULL); host or device arrays as
 * the context says.  RustpotterDetection::gain of a detection is the gain of the chunk in which its best window was scored
 * (src/detector.rs:411-414): with f = det.window + max_mfcc_frames - 1 the last frame of that window, chunk (f + fpf) / fpf counted
 * from the batch's first chunk (fpf = 3), i.e. the chunk whose frames contain f.  -1 before the first process call. */
int rp_stream_batch_levels(rp_stream_batch *b, float *rms, float *gains);

/* Live-stream batches whose detectors hold SEVERAL wakewords and / or wakeword MODELS (add_wakeword*, run_wakeword_detectors:
 * src/detector.rs:304-346,433-447): every wakeword whose own thresholds pass proposes a detection for the frame and the best
 * score wins; the window is as long as the longest wakeword and each wakeword scores its oldest frames
 * (wakeword_comp.rs:22-27, wakeword_nn.rs:137: truncate).  One entry per wakeword: exactly one of `templates` / `model`;
 * threshold / avg_threshold: a reference's own Option<f32> overrides, NaN = the value in `config`; none_index / precision as in
 * rp_batch_detect_model.  All wakewords share mfcc_size (else "Usage of wakewords with different mfcc size is not supported,
 * ignoring wakeword").  The batch borrows the context and every templates / model handle. */
typedef struct rp_model rp_model;
typedef struct {
    const rp_templates *templates;
    const rp_model *model;
    int none_index;
    int precision;
    float threshold;
    float avg_threshold;
} rp_wakeword_spec;
int rp_stream_batch_new_multi(rp_ctx *ctx, size_t n_wakewords, const rp_wakeword_spec *wakewords, int mfcc_size,
                              const rp_detector_config *config, size_t S, size_t max_chunks_per_call, rp_stream_batch **out);
/* rp_stream_batch_process that also tells which wakeword fired: det_wakeword [S][max_det] = index into `wakewords`,
 * det_label [S][max_det] = the label index when that wakeword is a model, else -1 (either may be NULL).  Works on every
 * stream batch (a batch of rp_stream_batch_new reports wakeword 0, label -1).  Fed the same audio piece by piece it gives
 * the detections of rp_batch_detect_multi / rp_batch_detect_model over the concatenation. */
int rp_stream_batch_process_multi(rp_stream_batch *b, const void *pcm, rp_sample_format fmt, size_t n_chunks, size_t pcm_stride,
                                  rp_batch_detection *det, int32_t *det_wakeword, int32_t *det_label, int32_t *n_det, int max_det);

/* Personal wakewords on LIVE streams: a live-stream batch over a wakeword bank -- enrol (rp_wakeword_ref_build_batch) -> bank -> live
 * detect, every stream's detector state on the device.  Stream s behaves as Rustpotter::new(config) + add_wakeword(bank[stream_wakeword[s]])
 * + process_samples per chunk: rp_batch_detect_bank's semantics with the state carried between calls -- its own window length (the
 * wakeword's longest sample template) and countdown max_len / 2, the wakeword's own thresholds over config's, the averaged-template test
 * only when the wakeword has an averaged template and its effective avg_threshold != 0.  stream_wakeword[s] == -1: a detector without
 * wakewords, which never reports.  Fed the same audio piece by piece a stream reports the detections of rp_batch_detect_bank over the
 * concatenation, bit for bit (with the last-bits exception of the bank calls above: a window with a frame outside the norm range of the
 * fast cosine within band_size - 2 frames behind its end may be rescored by one call and not the other; both within the parity bar).
 * The batch borrows `ctx` and `bank` (the bank must belong to `ctx`) and keeps its own device copy of the indices.  stream_wakeword [S]: a
 * host array under RP_CTX_HOST_POINTERS -- an index outside [-1, n_wakewords) is then an error that names the stream, found before
 * anything is allocated -- else a device array, copied; the kernels treat such an index as -1.  Every stream keeps an MFCC history of
 * rp_wakeword_bank_max_len(bank, -1) - 1 frames (of max(that, rp_wakeword_bank_reserved_len(bank)) - 1 for a reserved bank, which may then
 * change under the batch: see rp_wakeword_bank_reserve); the window ending at a new frame starts max_len(s) - 1 frames before it.
 * Limits as the bank calls: mfcc_size 5, 13 or 16 with band_size 3..6, or band_size 0 (every score 0, no detection); an empty bank or all
 * indices -1: calls succeed and report nothing.  Arithmetic: f32 vector FMAs whatever rp_ctx_set_arithmetic says (neither read nor
 * changed); rp_ctx_dtw_kernels reports RP_DTW_KERNEL_BANK_STREAM.
 * rp_stream_batch_process / _process_multi work on such a batch: agg [S][frames per call] is the score_mode aggregate of the stream's OWN
 * window ending at each new frame (a zero row for a stream without a wakeword; windows reaching before frame 0 are unspecified);
 * det_wakeword is the stream's bank index, det_label -1.  Without agg and without RP_CTX_FULL_SCORES a window below its avg_threshold is
 * not compared with the sample templates; the detections are the same either way.  rp_stream_batch_set_input works as on any batch.
 * rp_stream_batch_set_filters takes the band-pass filter alone: with gain_normalizer.enabled it fails (its one rms_level_ref has no
 * per-stream meaning); rp_stream_batch_set_filters_bank below gives every stream the gain normaliser of its own wakeword. */
int rp_stream_batch_new_bank(rp_ctx *ctx, const rp_wakeword_bank *bank, const int32_t *stream_wakeword, const rp_detector_config *config,
                             size_t S, size_t max_chunks_per_call, rp_stream_batch **out);
/* Connect / disconnect of device slots, at any time between process calls: streams first_stream .. first_stream + n - 1 get the indices
 * wakewords [n] (host or device array, checked as above; -1: none) and each is reset exactly as rp_stream_batch_reset(b, s) does
 * (add_wakeword on a detector without wakewords calls reset(), src/detector.rs:304-307; the filters' state and the resampler are not
 * touched).  A refused index changes nothing.  An error on a batch not made by rp_stream_batch_new_bank.
 * Replacing a wakeword in the bank (rp_wakeword_bank_put / _enrol) does not touch the streams that hold its index: they score the new
 * templates from the next call with the state they have.  Call this function for them to get remove_wakeword + add_wakeword. */
int rp_stream_batch_set_wakewords(rp_stream_batch *b, size_t first_stream, size_t n, const int32_t *wakewords);
/* rp_stream_batch_set_filters for a batch made by rp_stream_batch_new_bank (an error on any other): the gain normaliser of stream s works
 * towards the rms_level of ITS wakeword (rp_wakeword_bank_rms_level; filters->gain_normalizer.gain_ref for every stream when
 * has_gain_ref) over a window of max(max_len(s) / 3, 1) chunk levels, both read from the bank at the start of every process call.  The
 * rules of rp_stream_batch_set_filters hold: before the first audio, 30 ms chunks only, either order with rp_stream_batch_set_input;
 * rp_stream_batch_levels works as on any filtered batch; with the band-pass alone it is rp_stream_batch_set_filters.
 * A slot that changes wakeword (rp_stream_batch_set_wakewords) does what remove_wakeword + add_wakeword do (on_wakeword_change ->
 * set_rms_level_ref, gain_normalizer_filter.rs:42-48): new level and window size, the window of chunk levels is neither cleared nor
 * shortened -- filter() pushes one level and drops one only when the window is longer than window_size, so a window that was longer
 * keeps its length.  A stream with index -1 does not advance its window and has gain 1; connected again, its window goes on from what
 * it held.  rp_stream_batch_reset leaves the filters alone, as everywhere. */
int rp_stream_batch_set_filters_bank(rp_stream_batch *b, const rp_filters_config *filters);

/* Wakeword sets on LIVE streams: rp_stream_batch_new_bank with stream_wakewords [S][set_size] (see rp_batch_detect_bank_sets for what a
 * set means: add_wakeword x n per user, src/detector.rs:304-346,433-447).  Fed the same audio piece by piece a stream reports the
 * detections of rp_batch_detect_bank_sets over the concatenation.  History, reserve rules and the bank's count of batches are those of
 * rp_stream_batch_new_bank; the bank may change under the batch in the same way: Lmax(s) and every threshold are read from the bank in
 * every call.  rp_ctx_dtw_kernels reports RP_DTW_KERNEL_BANK_SETS_STREAM.
 * On such a batch rp_stream_batch_process works without agg (with agg it is refused: a batch of several wakewords has no single aggregate
 * per window; see rp_stream_batch_slot_scores), rp_stream_batch_process_multi reports det_wakeword = the winner's bank index and det_label
 * -1; rp_stream_batch_set_input, _reset and rp_stream_batch_set_filters with the band-pass alone work as on a bank batch;
 * rp_stream_batch_set_wakewords and rp_stream_batch_set_filters_bank fail; the gain normaliser of a sets batch comes with
 * rp_stream_batch_set_filters_per_stream (below the model sets). */
int rp_stream_batch_new_bank_sets(rp_ctx *ctx, const rp_wakeword_bank *bank, const int32_t *stream_wakewords, int set_size,
                                  const rp_detector_config *config, size_t S, size_t max_chunks_per_call, rp_stream_batch **out);
/* rp_stream_batch_set_wakewords for a sets batch (an error on any other), at any time between process calls: streams first_stream ..
 * first_stream + n - 1 get the rows stream_wakewords [n][set_size] and each is reset exactly as rp_stream_batch_set_wakewords resets.  A
 * refused row changes nothing.  This is remove-all plus add-in-order (remove_wakeword for every wakeword, then add_wakeword slot by slot:
 * the first add on the emptied detector resets it, src/detector.rs:304-307).  The reference's add_wakeword on a NON-empty detector, which
 * does not reset, is not offered. */
int rp_stream_batch_set_wakeword_sets(rp_stream_batch *b, size_t first_stream, size_t n, const int32_t *stream_wakewords);
/* The slot scores of the last process call of a sets batch, modelled on rp_stream_batch_levels: agg and avg [S][set_size][frames of that
 * call] (either may be NULL), the score of wakeword set[s][j] for the window of Lmax(s) frames that ends at each new frame, zero rows for
 * empty slots.  The windows are fully scored only under RP_CTX_FULL_SCORES; otherwise a window below its avg_threshold holds aggregate 0.
 * Returns -1 before the first process call and on a batch that is not a sets batch. */
int rp_stream_batch_slot_scores(rp_stream_batch *b, float *agg, float *avg);

/* A wakeword model (src/wakewords/wakeword_model.rs:11-18) resident on the device.  weights are
 * HOST arrays W_l [dims[l+1]][dims[l]] (candle Linear: x.W^T + b), biases b_l [dims[l+1]]; 1..3 layers. */
int rp_model_new(rp_ctx *ctx, int n_layers, const int *dims, const float *const *weights, const float *const *biases,
                 rp_model **out);
void rp_model_free(rp_model *m);

enum { RP_MLP_F32 = 0, RP_MLP_BF16 = 1, RP_MLP_F32_STRICT = 2, RP_MLP_F32_FAST = 3 };
/* WakewordNN forward (ModelImpl::forward: Linear -> ReLU -> ... -> Linear, raw logits),
 * src/wakewords/nn/wakeword_nn.rs:101-106,305-389: x [B][dims[0]] (the flattened, mean-normalised
 * window, :139-149,268-273) -> logits [B][dims[n_layers]].  Layer 1 runs on the matrix cores:
 * RP_MLP_F32 = f32-grade layer 1: inputs and weights as three bf16 parts each (exact: 3 x 8 = an f32's 24 significant bits), six of the
 *   nine partial products of a multiplication accumulated in f32 -- what is dropped is below 2^-22 of a product, 2^-25.7 rms (an f32
 *   multiply rounds by up to 2^-24); bf16 has the f32 exponent range, so there is no out-of-range row and no second pass; finite input
 *   never gives NaN logits.  (A feature that is +-inf splits into inf + NaN: that row's logits are NaN, where candle's f32 Linear would
 *   answer +-inf, NaN or -- every such product cut by the ReLU -- finite values; NaN features give NaN in both.)  A model whose three-part
 *   weight groups do not fit the LDS runs the f32 matrix instructions.
 * RP_MLP_F32_STRICT = the f32 matrix instructions for every row (each output a k-ordered fmaf chain, as candle's f32 Linear up to
 *   summation order).
 * RP_MLP_F32_FAST = two f16 parts per operand (22 significant bits, one partial product dropped: NARROWER than the reference's f32 products;
 *   logits within 1e-5), a row that holds a feature beyond the f16 range, |x| > 65 504, is computed by the f32 matrix instructions in a
 *   second short pass; the form the whole-stream window kernels of rp_batch_detect_model use at the matrix cores' full rate.
 * RP_MLP_BF16 = inputs rounded to bf16, f32 accumulate. */

int rp_mlp_forward_batch(rp_ctx *ctx, const rp_model *model, const float *x, size_t B, int precision, float *logits);

/* The same forward over EVERY window of S streams' MFCC rows, what WakewordNN::run_detection computes frame after frame
 * (src/wakewords/nn/wakeword_nn.rs:101-159: the window of train_size = dims[0] / mfcc_size frames, mean-normalised by
 * MfccNormalizer::normalize, flattened, through the model): mfcc [S][n_frames][mfcc_size] -> logits [S][n_win][dims[n_layers]],
 * n_win = n_frames - train_size + 1 (0 rows when a stream is shorter than a window).  The windows are never materialised: a
 * stream's frames are staged once and the window mean is taken out after layer 1 (W.(f - mu) = W.f - sum_k mu[k] wsum[k]);
 * RP_MLP_BF16 is accepted and computes as RP_MLP_F32 here (bf16 is an INPUT format of rp_mlp_forward_batch's dense rows).
 * From 32 windows on (mfcc_size 16) a workgroup stages its share of a stream -- at most 224 consecutive windows -- minus the mean of its
 * middle window: a frame far outside the others' range inside that window leaves the workgroup's OTHER windows right to 1e-5 of
 * |their mean - that mean| (about the frame's value / train_size), not of their own features.  The windows that hold the frame, the
 * stream's other workgroups and the other streams are not affected.
 * rp_batch_detect_model is this call between rp_mfcc_batch and the score / detection passes. */
int rp_mlp_forward_windows(rp_ctx *ctx, const rp_model *model, const float *mfcc, size_t S, size_t n_frames, int mfcc_size,
                           int precision, float *logits);

/* rp_batch_detect for a wakeword MODEL (WakewordNN::run_detection, src/wakewords/nn/wakeword_nn.rs:39-159, inside the
 * detection state machine): MFCC -> windows of train_size = dims[0] / mfcc_size frames, mean-normalised -> MLP forward
 * -> per window the arg-max label (the last maximum; `none_index` = index of the "none" label, -1 without one),
 * score = 1 - 1/(1 + exp(((label - none) - 10 score_ref) / (10 score_ref))), avg_score likewise against the smallest
 * other logit when config->avg_threshold != 0, kept when score >= threshold && avg_score >= avg_threshold -> state
 * machine.  precision: RP_MLP_F32 / RP_MLP_F32_STRICT / RP_MLP_BF16.  det_label [S][max_det] (NULL to skip): label index of a detection. */
int rp_batch_detect_model(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                          const rp_model *model, int mfcc_size, int none_index, const rp_detector_config *config, int precision,
                          rp_batch_detection *det, int32_t *det_label, int32_t *n_det, int max_det);

/* Personal wakeword MODELS: a model BANK -- W wakeword models resident on the device -- and whole-recording calls in which stream s runs its
 * own model stream_model[s].  The batched form of one `Rustpotter` per thread, each holding one wakeword model; the model counterpart of
 * rp_wakeword_bank.  The bank COPIES what it needs of every model (device to device), so the rp_model handles may be freed once the bank
 * exists; it borrows `ctx`, which must outlive it, and is used with that context only.  A model has no thresholds of its own
 * (run_wakeword_detectors, src/detector.rs:433-447, passes the detector's): every stream takes the call's config.
 * Limits (refused with an error that names them) -- the shapes whose whole-recording forward is mlp_windows_kernel: mfcc_size 16 with an
 * input of whole frames; windows (train_size) of at most 256 frames; layer 1 at most 32 wide (every Tiny model, Small models up to 197
 * frames); tail layers at most 32 wide; a packed tail of at most 6144 floats.  Medium and Large models are refused.  Within the limits a
 * bank may mix window lengths, widths, layer counts and label counts freely.  An empty bank (n_models == 0) is a Rustpotter without
 * wakewords: calls succeed with every index -1, report no detection and write zero rows.
 * Arithmetic: RP_MLP_F32 (three bf16 parts) only, one forward launch per call; RP_MLP_BF16 is accepted and computes the same, as in
 * rp_mlp_forward_windows; RP_MLP_F32_FAST and RP_MLP_F32_STRICT are refused.  rp_ctx_last_mlp_kernel reports
 * "mlp_windows_bank_kernel<bf16x3 splits>".
 * BITS: a stream is cut into workgroups from its OWN window count n_win(s) = n_frames - train_size(s) + 1 by the rule of the shared-model
 * path, so a bank call gives stream s exactly the bits rp_mlp_forward_windows / rp_batch_detect_model give that stream alone with its model
 * under RP_MLP_F32, in any batch, order and mixture -- whenever n_win(s) >= 32.  (One exception, in the last bits only: a stream with fewer
 * than 32 windows is one partial tile of the same kernel here, where the shared-model path reads such windows in place with each window's
 * own mean, mlp_mfma_kernel; the two agree within 2e-6 on scores, the figure of INTEGRATION.md section 3 for that pair of kernels, and
 * both are within the parity bar.) */
typedef struct rp_model_bank rp_model_bank;
/* models [n_models]: handles of this context.  none_index [n_models]: index of each model's "none" label, -1 without one (NULL: every -1).
 * A model that is refused fails the call with "model <index>: <reason>". */
int rp_model_bank_new(rp_ctx *ctx, size_t n_models, const rp_model *const *models, int mfcc_size, const int32_t *none_index, rp_model_bank **out);
/* The same from wakeword-model .rpw bytes (what rp_wakeword_model_train returns): the layers by model type, none_index from the labels,
 * mfcc_size from the files -- all equal, else "wakeword <index>: Usage of wakewords with different mfcc size is not supported, ignoring
 * wakeword" (src/detector.rs:310-320).  A wakeword reference or a file the reader refuses fails the call: "wakeword <index>: <reason>". */
int rp_model_bank_new_from_rpw(rp_ctx *ctx, size_t n_models, const uint8_t *const *rpw_buffers, const size_t *rpw_lens, rp_model_bank **out);
void rp_model_bank_free(rp_model_bank *bank);
/* models in the bank; -1 for a NULL bank */
int rp_model_bank_size(const rp_model_bank *bank);
/* train_size (the window length in frames) of one model; model < 0: the largest in the bank (0 for an empty bank).  -1 for a NULL bank or
 * an index outside the bank. */
int rp_model_bank_train_size(const rp_model_bank *bank, long long model);
/* label count of one model; model < 0: the label pitch of rp_mlp_forward_windows_bank and rp_stream_batch_logits = max(reserved label count,
 * the largest in the bank), so the largest in the bank for a bank nobody reserved (while a stream batch over the bank exists the pitch
 * never shrinks: a replaced model may leave it larger than the bank needs until the batches are gone and the next put).  -1 as above. */
int rp_model_bank_labels(const rp_model_bank *bank, long long model);
/* ---- A model bank that changes: train, add and replace models, also under live-stream batches.  The model counterpart of "A bank that
 * changes" above (rp_wakeword_bank_reserve / _put / _put_from_rpw / _enrol).
 * rp_model_bank_put / _put_from_rpw / _train write the models first .. first + n - 1.  first <= rp_model_bank_size is required (a bank has no
 * holes): indices below the size are REPLACED, indices at or above it extend the bank; n == 0 succeeds and changes nothing.  Every limit and
 * wording of rp_model_bank_new applies per model ("model <index>: <reason>", <index> = the bank index first + i; the .rpw route says
 * "wakeword <index>: <reason>" as rp_model_bank_new_from_rpw does).  These calls also refuse parameters that are not finite ("model <index>:
 * parameters must be finite"); rp_model_bank_new stays as it is.  A call that is refused or fails leaves the bank exactly as it was: size,
 * largest window, label pitch, every image byte.
 * The models' bank images are built ON THE DEVICE from the raw f32 parameters (model_bank_put_kernel, one launch per call whatever n) with
 * exactly the bits rp_model_bank_new gives them: the three-part bf16 image of layer 1, its bias, the per-coefficient weight sums and the
 * packed tail layers.
 * Storage: the bank's device arrays are pools.  New entries are appended, a replaced model's old ones stay behind as garbage, and a full pool
 * is replaced by one of at least twice the size into which only the live models move (on the device) -- growth is the compaction.
 * Ordering: every update is enqueued on the context's stream behind whatever still reads the bank, and the call returns after it has
 * completed.  The next call that uses the bank sees the new contents, the next rp_stream_batch_process of a live batch over it included;
 * nothing in flight ever sees a half-written model, and an old pool is freed only after the move out of it has completed.
 * Live-stream batches: a model-bank batch sizes every stream's MFCC history (the largest train_size - 1 frames) and its logits (the label
 * pitch) once, at creation, and keeps both as its own from then on; so the bank must never come to hold a window longer or a label count
 * larger than a live batch has room for.  rp_model_bank_reserve declares the largest the bank will ever hold: a put refuses what exceeds it,
 * and rp_stream_batch_new_model_bank keeps room for max(reserved, current, 1).  Without a reservation, while a batch over the bank exists, a
 * window longer or a label count larger than the current largest is refused (the error says to call rp_model_bank_reserve before creating the
 * batch); without either, anything within the bank's limits goes.  The bank counts its batches (a batch is freed before its bank).  A
 * reserved bank of 0 models is the natural starting state of a service.
 * The bank does not touch batches: a stream that holds an index while that index is replaced runs the new model from the next call on, with
 * the detector state it has; its window becomes the new train_size, read from the history the stream already holds.  For the reference's
 * remove_wakeword + add_wakeword, call rp_stream_batch_set_models for those streams: it resets them as it always does.  Removing a model is not
 * offered: disconnect its streams; the next put reuses the slot.
 * All host arrays of these calls are HOST arrays, whatever the pointer flag of the context. */
/* max_train_size > 0: no model's window may become longer; at least the current largest, at most 256.  max_labels > 0: no model may have more
 * labels; at least the current largest, at most 32 (the limit on tail-layer width).  Both can change only while no stream batch over the bank
 * exists; 0 leaves a value as it is.  n_models / n_frames (the sum of the models' windows) pre-size the pools; hints, never limits. */
int rp_model_bank_reserve(rp_model_bank *bank, int max_train_size, int max_labels, size_t n_models, size_t n_frames);
/* the reserved train size and label count (either pointer may be NULL), 0 = none; returns 0, -1 for a NULL bank */
int rp_model_bank_reserved(const rp_model_bank *bank, int *max_train_size, int *max_labels);
/* how often the pools have been replaced by larger ones so far (tests and capacity planning); -1 for a NULL bank */
int rp_model_bank_pool_growths(const rp_model_bank *bank);
/* models [n]: handles of the bank's context, read through their raw device parameters; none_index [n] as in rp_model_bank_new. */
int rp_model_bank_put(rp_model_bank *bank, size_t first, size_t n, const rp_model *const *models, const int32_t *none_index);
/* The same from wakeword-model .rpw bytes, with the rules of rp_model_bank_new_from_rpw (one mfcc_size, 16): the files are parsed on the host,
 * the raw parameters of all n models go to the device in one upload, and no rp_model is created. */
int rp_model_bank_put_from_rpw(rp_model_bank *bank, size_t first, size_t n, const uint8_t *const *rpw_buffers, const size_t *rpw_lens);
/* Training straight into bank slots: the arguments of rp_wakeword_model_train_batch from `seeds` on, unchanged, and the same stages; the
 * trained parameters then go from the training workspace into the bank on the device -- no parameter round trip.  Labels, none_index and
 * train_size are the trained model's.  options->mfcc_size other than 16, or a previous model of another mfcc_size, is refused with the bank's
 * wording; a training set the single call refuses fails the call with that error behind "model <index>: " (the bank index); a model that
 * trains to parameters that are not finite fails it with "model <index>: parameters must be finite".  out_rpw / out_lens [n] may both be
 * NULL; given, they receive exactly rp_wakeword_model_train_batch's bytes (free each with rp_buffer_free), and on failure every entry is
 * NULL. */
int rp_model_bank_train(rp_model_bank *bank, size_t first, size_t n, const rp_train_options *options, const uint64_t *seeds,
                        const size_t *train_counts, const char *const *train_names, const uint8_t *const *train_wavs, const size_t *train_lens,
                        const size_t *test_counts, const char *const *test_names, const uint8_t *const *test_wavs, const size_t *test_lens,
                        const uint8_t *const *prev_models, const size_t *prev_model_lens, uint8_t **out_rpw, size_t *out_lens, float *final_loss,
                        float *test_accuracy);
/* The bank image of one model as the kernels read it, copied to the HOST buffer `out` of `cap` bytes: wimg (train_size * 192 pieces of 16
 * bytes, [frame][part 3][k-half][output < 32][8 k] bf16) | b1 | wsum [rows][16] | tail, zero padded to a multiple of 4 floats.  *need (may
 * be NULL) receives the byte count; out == NULL only queries it.  It exists so that the prepared bits can be compared directly. */
int rp_model_bank_read_image(const rp_model_bank *bank, long long model, void *out, size_t cap, size_t *need);
/* model_bank_put_kernel's own time in the bank's last put, in milliseconds, by events around its launch; 0 unless the context times its
 * kernels (rp_ctx_timing_enable).  0 for a NULL bank. */
double rp_model_bank_last_put_ms(const rp_model_bank *bank);
/* rp_mlp_forward_windows with stream s run by model stream_model[s] [S] (-1: none): mfcc [S][n_frames][16] ->
 * logits [S][win_pitch][rp_model_bank_labels(bank, -1)].  Row (s, w) holds the labels of s's model, zeros behind them; windows behind
 * n_win(s), streams without a model and streams shorter than their window are zero rows.  win_pitch below the largest n_win(s) of the call
 * is refused (device arrays: below the largest window count any model of the bank has).  Indices: with RP_CTX_HOST_POINTERS an index outside
 * [-1, W) is an error that names the stream, found before anything is launched or written; with device arrays the kernels treat such an
 * index as -1. */
int rp_mlp_forward_windows_bank(rp_ctx *ctx, const rp_model_bank *bank, const int32_t *stream_model, const float *mfcc, size_t S, size_t n_frames,
                                int precision, float *logits, size_t win_pitch);
/* rp_batch_detect_model with stream s run by model stream_model[s]: stream s behaves as Rustpotter::new(config) +
 * add_wakeword(models[stream_model[s]]) + process_samples -- its window is its model's train_size, its countdown train_size / 2; VAD, reset
 * and the score / label logic as in rp_batch_detect_model, none_index from the bank.  A stream with index -1, or shorter than its window,
 * reports n_det = 0.  det_label [S][max_det] (NULL to skip): label index of each detection, 0 behind a stream's detections (as
 * rp_batch_detect_model).  Index rules as rp_mlp_forward_windows_bank.  Every detection equals that of rp_batch_detect_model over the
 * stream alone with its model (scores bit for bit under BITS above). */
int rp_batch_detect_model_bank(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                               const rp_model_bank *bank, const int32_t *stream_model, const rp_detector_config *config, int precision,
                               rp_batch_detection *det, int32_t *det_label, int32_t *n_det, int max_det);

/* Personal wakeword models on LIVE streams: a live-stream batch in which stream s runs its own model bank[stream_model[s]] [S] (-1: none).
 * Stream s behaves as Rustpotter::new(config) + add_wakeword(models[stream_model[s]]) + process_samples per chunk -- the semantics of
 * rp_batch_detect_model_bank with the detector state carried between calls on the device.  Thresholds come from `config` (a model has none of
 * its own), mfcc_size is 16, the arithmetic is RP_MLP_F32, and a process call makes ONE forward launch (mlp_bank_stream_kernel) whatever
 * the number of models.  Every stream keeps a history of max(reserved, rp_model_bank_train_size(bank, -1), 1) - 1 frames; its own window starts
 * train_size(s) - 1 frames before the new frame.  Index rules are those of rp_stream_batch_new_bank: a host array is checked before
 * anything is allocated (an index outside [-1, W) is an error that names the stream), a device array is copied and the kernels treat such
 * an index as -1.  An empty bank, or every index -1: calls succeed and report nothing.  The batch borrows `ctx` and `bank`, which must
 * outlive it; the bank must belong to `ctx`.
 * BITS: every window is computed row by row with the arithmetic of mlp_mfma_kernel's three-part form reading the window in place with its
 * own mean -- what rp_mlp_forward_windows gives for fewer than 32 windows and what a shared-model live batch (rp_stream_batch_new_multi)
 * gives for fewer than 32 new windows a call.  So a stream's logits, scores and detections do not depend on how the caller cuts the audio
 * into calls, on the batch or on the stream's place in it, and equal those of rp_stream_batch_new_multi with that one model (calls of at
 * most 10 chunks).  Against rp_batch_detect_model_bank over the concatenation (mlp_windows_bank_kernel, frames staged relative to a
 * workgroup's middle window): equal detections, scores within 2e-6.
 * On such a batch rp_stream_batch_process works without agg (with agg it is refused: the per-window output is the logits, see
 * rp_stream_batch_logits); rp_stream_batch_process_multi reports det_wakeword = the stream's model index and det_label = the label index
 * of the detection's best window; rp_stream_batch_set_input, _reset and _chunks_seen work as everywhere; rp_stream_batch_set_filters takes
 * the band-pass filter alone (with the gain normaliser enabled it is refused; rp_stream_batch_set_filters_per_stream gives every stream the
 * gain normaliser of its own model); VAD works as on every live batch.  rp_stream_batch_set_wakewords, _set_wakeword_sets, _set_filters_bank and _slot_scores are refused with an error that says
 * why. */
int rp_stream_batch_new_model_bank(rp_ctx *ctx, const rp_model_bank *bank, const int32_t *stream_model, const rp_detector_config *config, size_t S,
                                   size_t max_chunks_per_call, rp_stream_batch **out);
/* Connect, disconnect and retarget slots of a model-bank batch, at any time between process calls: streams first_stream .. first_stream +
 * n - 1 get the model indices models [n] (-1: none) and each is reset exactly as rp_stream_batch_set_wakewords resets.  A refused index
 * (host arrays) names its stream and changes nothing.  An error on any other kind of batch. */
int rp_stream_batch_set_models(rp_stream_batch *b, size_t first_stream, size_t n, const int32_t *models);
/* The logits of the last process call of a model-bank batch, modelled on rp_stream_batch_slot_scores: logits [S][frames of that
 * call][rp_model_bank_labels(bank, -1)], row (s, i) for the window of train_size(s) frames that ends at new frame i.  Values behind a
 * model's labels are zero, rows of streams without a model are zero.  Windows that reach before frame 0 or before the stream's last reset
 * are unspecified.  Returns -1 before the first process call and on any other kind of batch. */
int rp_stream_batch_logits(rp_stream_batch *b, float *logits);

/* Model SETS: several personal wakeword models per stream over a model bank.  stream_models [S][set_size] (set_size 1..RP_MODEL_SET_MAX) holds
 * bank indices, -1 an empty slot anywhere in a row; stream s behaves as Rustpotter::new(config), add_wakeword(models[i]) for each live slot
 * of its row in slot order, process_samples (src/detector.rs:304-346, 433-447, wakeword_nn.rs:137):
 *  - its window is Lmax(s) frames, the longest train_size of its live slots, its countdown Lmax(s) / 2; it has n_win_s = n_frames - Lmax(s) + 1
 *    windows;
 *  - slot j scores the OLDEST train_size(j) frames of that window, with the thresholds of `config` (a model has none of its own; >=);
 *  - the best passing score wins, the first slot of equal scores; a detection reports window = frame - Lmax(s) + 1, the winner's BANK index
 *    and the label index of its best window.
 * A row of all -1 is a detector without wakewords; duplicate indices change nothing.  Limits, arithmetic (RP_MLP_F32; RP_MLP_BF16 computes
 * the same; the others are refused), empty-bank behaviour and index rules are those of the model-bank calls: with RP_CTX_HOST_POINTERS an index
 * outside [-1, W) is an error that names the stream and the slot, found before anything is allocated or launched; with device arrays the
 * kernels treat such an index as -1. */
enum { RP_MODEL_SET_MAX = 8 };
/* rp_mlp_forward_windows_bank over sets: logits [S][set_size][win_pitch][rp_model_bank_labels(bank, -1)]; row (s, j, w) holds model
 * stream_models[s][j] on the train_size(j) frames from frame w, for w < n_win_s.  Rows are zero behind a model's labels, behind n_win_s, in
 * empty slots and in EVERY slot of a stream shorter than Lmax(s), even where a shorter model of the set would fit (as
 * rp_dtw_score_bank_sets).  win_pitch rules as rp_mlp_forward_windows_bank.  BITS: row (s, j) equals rp_mlp_forward_windows_bank over the
 * first n_frames - (Lmax(s) - train_size(j)) frames of stream s with that model alone (the same kernel body with the same cut). */
int rp_mlp_forward_windows_bank_sets(rp_ctx *ctx, const rp_model_bank *bank, const int32_t *stream_models, int set_size, const float *mfcc, size_t S,
                                     size_t n_frames, int precision, float *logits, size_t win_pitch);
/* rp_batch_detect_model_bank over sets.  det_model / det_label [S][max_det] (NULL to skip): each detection's bank index and label index;
 * behind a stream's detections 0 and -1.  VAD and the reset after a detection as everywhere. */
int rp_batch_detect_model_bank_sets(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                                    const rp_model_bank *bank, const int32_t *stream_models, int set_size, const rp_detector_config *config,
                                    int precision, rp_batch_detection *det, int32_t *det_model, int32_t *det_label, int32_t *n_det, int max_det);
/* Model sets on LIVE streams: rp_stream_batch_new_model_bank with stream_models [S][set_size].  History, reservation rules, the bank's count
 * of batches and the behaviour under rp_model_bank_put / _put_from_rpw / _train are those of rp_stream_batch_new_model_bank; Lmax(s) is read
 * from the bank in every call.  A process call makes ONE forward launch (mlp_set_stream_kernel) over (stream, slot, row tile); the first
 * window of a call starts Lmax(s) - 1 frames before the first new frame for every slot.  A stream fed in pieces reports the detections of
 * rp_batch_detect_model_bank_sets over the concatenation, scores within 2e-6; its logits do not depend on the cut
 * into calls and equal, slot by slot, those of rp_stream_batch_new_multi with the live slots' models (calls of at most 10 chunks).
 * rp_stream_batch_process works without agg and is refused with agg; rp_stream_batch_process_multi reports det_wakeword = the winner's bank
 * index and det_label; rp_stream_batch_logits returns [S][set_size][frames of the call][label pitch]; rp_stream_batch_set_input, _reset,
 * _chunks_seen and the band-pass-only rp_stream_batch_set_filters work as on a model-bank batch.  The gain normaliser through
 * rp_stream_batch_set_filters, _set_models, _set_wakewords, _set_wakeword_sets, _set_filters_bank and _slot_scores are refused, each with an
 * error that says why; rp_stream_batch_set_filters_per_stream gives such a batch the gain normaliser. */
int rp_stream_batch_new_model_bank_sets(rp_ctx *ctx, const rp_model_bank *bank, const int32_t *stream_models, int set_size,
                                        const rp_detector_config *config, size_t S, size_t max_chunks_per_call, rp_stream_batch **out);
/* Re-target streams first_stream .. first_stream + n - 1 of such a batch: stream_models [n][set_size].  All slots are removed, the new ones
 * added in order and the stream reset, as rp_stream_batch_set_wakeword_sets does.  A refused row (host arrays) names its stream and slot and
 * changes nothing.  An error on any other kind of batch. */
int rp_stream_batch_set_model_sets(rp_stream_batch *b, size_t first_stream, size_t n, const int32_t *stream_models);

/* The gain normaliser where a stream holds SEVERAL entries of a bank, or a model.  A Rustpotter with several wakewords works towards the
 * largest rms_level of its wakewords, NaN ignored (f32::max folded from NaN; NaN when none has a level: gain 1), over a window of
 * max_mfcc_frames / 3 chunk levels, at least 1 (on_wakeword_change, src/detector.rs:328-338; set_rms_level_ref,
 * gain_normalizer_filter.rs:42-48).  For stream s that is target(s) = the largest non-NaN level and Lmax(s) = the longest window over the
 * live slots of its row; one short kernel (stream_targets_kernel) prepares both per stream in front of the per-stream gain kernels of
 * rp_frontend_batch_bank and rp_stream_batch_set_filters_bank, which are unchanged.  A model's level is part of the model bank:
 * WakewordModel::rms_level, kept from the .rpw files by rp_model_bank_new_from_rpw / _put_from_rpw, the level of the trained file after
 * rp_model_bank_train (rustpotter's trainer: the running mean of the non-"none" samples' levels), NaN for models given as handles
 * (rp_model_bank_new / _put).  It moves with the model when the bank's pools grow.
 * rms_levels: a HOST array [rp_model_bank_size], NaN allowed, whatever the pointer flag of the context; the write is ordered on the
 * context's stream and holds from the next call that uses the bank (rp_frontend_batch_model_bank, a live-stream batch with
 * rp_stream_batch_set_filters_per_stream). */
int rp_model_bank_set_rms_levels(rp_model_bank *bank, const float *rms_levels);
/* ... of one model as last set; NaN for a NULL bank or an index outside the bank. */
float rp_model_bank_rms_level(const rp_model_bank *bank, long long model);
/* rp_frontend_batch_bank for wakeword sets, what goes in front of rp_batch_detect_bank_sets: stream s works towards target(s) over
 * max(Lmax(s) / 3, 1) chunk levels (filters->gain_normalizer.gain_ref for every stream when has_gain_ref).  A row without a live slot is a
 * detector without wakewords: gain 1 for every chunk, the band-pass as on any stream.  stream_wakewords [S][set_size] as in
 * rp_dtw_score_bank_sets: with RP_CTX_HOST_POINTERS an index outside [-1, n_wakewords) is an error that names stream and slot, found before
 * anything is launched or written; with device arrays such an index counts as -1.  With set_size 1 the bits of rp_frontend_batch_bank. */
int rp_frontend_batch_bank_sets(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                                const rp_filters_config *filters, const rp_wakeword_bank *bank, const int32_t *stream_wakewords, int set_size,
                                float *pcm_out, size_t out_stride, float *rms, float *gains);
/* ... for a model bank, in front of rp_batch_detect_model_bank (set_size 1) and rp_batch_detect_model_bank_sets: stream_models
 * [S][set_size] as in rp_mlp_forward_windows_bank_sets, the level of a slot is rp_model_bank_rms_level, its window the model's train_size. */
int rp_frontend_batch_model_bank(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                                 const rp_filters_config *filters, const rp_model_bank *bank, const int32_t *stream_models, int set_size,
                                 float *pcm_out, size_t out_stride, float *rms, float *gains);
/* rp_stream_batch_set_filters for every batch over a bank: rp_stream_batch_new_bank_sets, rp_stream_batch_new_model_bank,
 * rp_stream_batch_new_model_bank_sets, and rp_stream_batch_new_bank, where it gives the bits of rp_stream_batch_set_filters_bank (a set of
 * one).  An error on a batch of shared wakewords (rp_stream_batch_new / _new_multi: rp_stream_batch_set_filters is theirs).  The gain
 * normaliser of stream s works towards target(s) over max(Lmax(s) / 3, 1) chunk levels (gain_ref for every stream when has_gain_ref); both
 * are prepared from the batch's indices and the bank at the start of EVERY process call, so a bank that changed under the batch
 * (rp_wakeword_bank_put / _enrol / _set_rms_levels, rp_model_bank_put / _put_from_rpw / _train / _set_rms_levels) is seen from the next call.
 * The ring of a stream has room for the bank's largest window (or its reservation), as on a one-wakeword bank batch.
 * The rules of rp_stream_batch_set_filters[_bank] hold: before the first audio, 30 ms chunks only, either order with
 * rp_stream_batch_set_input; rp_stream_batch_levels reports each chunk's level and gain; with the band-pass alone it behaves as
 * rp_stream_batch_set_filters; a refused call leaves the batch as it was.
 * Retargeting (rp_stream_batch_set_wakewords, _set_wakeword_sets, _set_models, _set_model_sets) does what remove-all plus add-in-order do in
 * the reference: the stream gets its new level and window size, the window of chunk levels is neither cleared nor shortened
 * (gain_normalizer_filter.rs:42-48), a stream left without a live slot has gain 1 and keeps its window for later.  rp_stream_batch_reset
 * leaves the filters alone, as everywhere. */
int rp_stream_batch_set_filters_per_stream(rp_stream_batch *b, const rp_filters_config *filters);

/* MIXED sets: wakeword references and wakeword models together on one stream, over whole recordings.  Stream s carries two rows:
 * stream_wakewords[s][0 .. ref_set_size) indexes a wakeword bank, stream_models[s][0 .. model_set_size) a model bank.  Each size is
 * 0 .. 8; a size of 0 (the array may then be NULL) means that side is absent; -1 is an empty slot anywhere in a row; duplicates change
 * nothing.  Stream s behaves as Rustpotter::new(config), add_wakeword for its live reference slots in slot order, then add_wakeword for its
 * live model slots in slot order, then process_samples (src/detector.rs:304-346, 433-447):
 *  - its window is Lmax(s) frames, the longest over the live slots of BOTH rows (max_len of a reference, train_size of a model), its
 *    countdown Lmax(s) / 2, and it has n_win_s = n_frames - Lmax(s) + 1 windows; a stream shorter than Lmax(s) reports nothing, even where a
 *    shorter wakeword of its set would fit;
 *  - every slot scores the OLDEST frames of that window, as many as its own length (wakeword_comp.rs:22-27, wakeword_nn.rs:137);
 *  - a reference proposes under its own thresholds over the config's (>), its averaged-template test as in rp_batch_detect_bank_sets; a
 *    model proposes under the config's thresholds (>=): the rules of the two families;
 *  - the best passing score wins; of equal scores the first in that order: references before models, slot order within a kind;
 *  - a detection reports window = frame - Lmax(s) + 1; det_wakeword is the winner's index in ITS OWN bank; det_label is the label index
 *    of the winner's best window for a model and -1 for a reference, so det_label >= 0 says that a model won.  Behind a stream's
 *    detections det_wakeword is 0 and det_label -1.
 * A stream with no live slot in either row is a detector without wakewords.  With every model slot -1 (or model_set_size 0) a stream
 * reports exactly what rp_batch_detect_bank_sets reports, with every reference slot -1 exactly what rp_batch_detect_model_bank_sets reports.
 * Both banks belong to the call's context.  The wakeword bank must have mfcc_size 16, which is what a model bank is; any other size fails
 * with "Usage of wakewords with different mfcc size is not supported, ignoring wakeword".  band_size 3..6, or 0.  Arithmetic is that of the
 * two families: references in f32 vector FMAs whatever rp_ctx_set_arithmetic says, models RP_MLP_F32 (RP_MLP_BF16 computes the same; the
 * others are refused).  Index rules are those of the two families: with RP_CTX_HOST_POINTERS an index outside its bank is an error that
 * names stream, slot and side ("wakeword index" / "model index"), found before anything is allocated or launched; with device arrays it
 * counts as -1.  Two empty banks, or rows of all -1: the call succeeds and reports nothing.  VAD and the reset after a detection as
 * everywhere.  rp_ctx_dtw_kernels reports RP_DTW_KERNEL_BANK_SETS: the call runs dtw_set_kernel and the model-set forward as they are, one
 * short kernel (stream_targets_kernel) folds Lmax(s) per stream, and one scan (scan_mixed_set_kernel) reads both kinds' proposals. */
int rp_batch_detect_mixed_sets(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                               const rp_wakeword_bank *bank, const int32_t *stream_wakewords, int ref_set_size, const rp_model_bank *model_bank,
                               const int32_t *stream_models, int model_set_size, const rp_detector_config *config, int precision,
                               rp_batch_detection *det, int32_t *det_wakeword, int32_t *det_label, int32_t *n_det, int max_det);
/* rp_frontend_batch_bank_sets with both rows and both banks, what goes in front of rp_batch_detect_mixed_sets: stream s works towards the
 * largest non-NaN rms_level over the live slots of BOTH rows (on_wakeword_change, src/detector.rs:328-338) over max(Lmax(s) / 3, 1) chunk
 * levels; gain_ref for every stream when has_gain_ref; a stream without a live slot, or with every level NaN, has gain 1.  Rows, sizes,
 * index rules and the mfcc_size rule as in rp_batch_detect_mixed_sets. */
int rp_frontend_batch_mixed_sets(rp_ctx *ctx, const void *pcm, rp_sample_format fmt, size_t S, size_t n_samples, size_t pcm_stride,
                                 const rp_filters_config *filters, const rp_wakeword_bank *bank, const int32_t *stream_wakewords, int ref_set_size,
                                 const rp_model_bank *model_bank, const int32_t *stream_models, int model_set_size, float *pcm_out,
                                 size_t out_stride, float *rms, float *gains);
/* Mixed sets on LIVE streams: rp_batch_detect_mixed_sets with the state carried between calls.  History per stream is the larger of what a
 * bank-sets batch and a model-sets batch would keep, reservations included; both banks count the batch, and both may change under it by
 * rp_wakeword_bank_put / _put_from_rpw / _enrol and rp_model_bank_put / _put_from_rpw / _train within what the batch was sized for: Lmax(s),
 * every threshold and the gain normaliser's level are read from the banks at the start of EVERY process call (stream_targets_kernel), so a
 * changed bank is seen from the next call.  A process call scores the reference slots with dtw_mixed_stream_kernel (rp_ctx_dtw_kernels reports
 * RP_DTW_KERNEL_MIXED_SETS_STREAM and only that bit) and the model slots with ONE forward launch (mlp_mixed_stream_kernel); the window that
 * ends at a new frame starts Lmax(s) - 1 frames before it for every slot of either kind.  A stream fed in pieces reports the detections of
 * rp_batch_detect_mixed_sets over the concatenation: frame, window, counter, det_wakeword and det_label exact, reference scores within 1e-5,
 * model scores within 2e-6; the kind of a partial detection is carried between calls with it.
 * rp_stream_batch_process works without agg and is refused with agg; rp_stream_batch_process_multi reports det_wakeword (the winner's index
 * in its own bank) and det_label (>= 0: a model won); rp_stream_batch_slot_scores answers the reference slots, [S][ref_set_size][frames of the
 * call]; rp_stream_batch_logits the model slots, [S][model_set_size][frames of the call][label pitch]; rp_stream_batch_set_filters_per_stream
 * gives the gain normaliser over both rows; rp_stream_batch_set_input, _reset, _chunks_seen and the band-pass-only
 * rp_stream_batch_set_filters work.  rp_stream_batch_set_wakewords, _set_wakeword_sets, _set_models, _set_model_sets, _set_filters_bank and
 * the gain normaliser through rp_stream_batch_set_filters are refused, each with an error that says why. */
int rp_stream_batch_new_mixed_sets(rp_ctx *ctx, const rp_wakeword_bank *bank, const int32_t *stream_wakewords, int ref_set_size,
                                   const rp_model_bank *model_bank, const int32_t *stream_models, int model_set_size,
                                   const rp_detector_config *config, size_t S, size_t max_chunks_per_call, rp_stream_batch **out);
/* Re-target streams first_stream .. first_stream + n - 1 of such a batch: stream_wakewords [n][ref_set_size] and stream_models
 * [n][model_set_size] (the sizes of the batch; NULL for a size of 0).  All slots of both rows are removed, the new ones added in order --
 * references, then models -- and the stream reset, as rp_stream_batch_set_wakeword_sets does.  A refused row (host arrays) names its stream,
 * slot and side and changes nothing.  An error on any other kind of batch. */
int rp_stream_batch_set_mixed_sets(rp_stream_batch *b, size_t first_stream, size_t n, const int32_t *stream_wakewords, const int32_t *stream_models);

/* Synthetic benchmark input of BASELINE.md §2, generated on the device:
 * pcm[s][i] = (splitmix64(seed ^ ((first_stream+s)<<32 + i)) >> 40) / 2^24 - 0.5 */
int rp_synth_pcm_batch(rp_ctx *ctx, uint64_t seed, uint64_t first_stream, size_t S, size_t n_samples, size_t pcm_stride,
                       float *pcm);

/* Average duration in ms of the launches of one kernel since the last reset, timed
 * with hipEvents on the launch stream (used by bench.py's roofline block).
 * kernel: 0 mfcc, 1 dtw, 2 aggregate, 3 scan, 4 mlp, 5 resample. */
int rp_ctx_timing_enable(rp_ctx *ctx, int enable);
int rp_ctx_timing_read(rp_ctx *ctx, int kernel, double *avg_ms, int *launches);
int rp_ctx_timing_reset(rp_ctx *ctx);

const char *rp_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RUSTPOTTER_HIP_H */
