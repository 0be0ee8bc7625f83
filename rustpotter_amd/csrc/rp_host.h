// rp_host.h -- host side of librustpotter_hip: constant tables, .rpw reader, device
// context, and the C++ mirror of the reference's `Rustpotter` (src/detector.rs).
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <exception>
#include <map>
#include <thread>
#include <tuple>
#include <memory>
#include <string>
#include <vector>

#include "../../include/rustpotter_hip.h"
#include "rp_kernels.h"

namespace rp {

// ---------------------------------------------------------------- constant tables
struct HostTables {
    int K1 = 0;
    std::vector<float> hamming, fb, dct;
    std::vector<float2> tw240, tw480;
    std::vector<int> centres;
};
// MfccExtractor::new / set_out_size(K) tables, src/mfcc/extractor.rs:19-59,115-120,164-198
HostTables build_tables(int K);

// ------------------------------------------------------------------- .rpw reader
struct WakewordRefData {  // src/wakewords/wakeword_ref.rs:12-20 (+ wakeword_v2.rs:8-16)
    std::string name;
    std::vector<std::string> tnames;  // file order
    std::vector<int> lens;
    std::vector<std::vector<float>> feats;  // [T] -> [len*K]
    bool has_avg = false;
    int avg_len = 0;
    std::vector<float> avg;
    bool has_threshold = false, has_avg_threshold = false;
    float threshold = 0.f, avg_threshold = 0.f;
    float rms_level = 0.f;
    int mfcc_size = 0;
};
struct WakewordModelData {  // src/wakewords/wakeword_model.rs:11-18,68-72
    std::vector<std::string> labels;
    size_t train_size = 0;
    int mfcc_size = 0;
    std::string m_type;
    std::map<std::string, std::pair<std::vector<size_t>, std::vector<float>>> weights;  // name -> (dims, data)
    float rms_level = 0.f;
};
enum class RpwKind { Ref, Model };
// WakewordV2 -> WakewordRef -> WakewordModel fall-through of src/detector.rs:152-176
bool parse_rpw(const uint8_t *buf, size_t len, RpwKind *kind, WakewordRefData *ref, WakewordModelData *model,
               std::string *err);

// ---------------------------------------------------------------- device context
struct Ctx;
// builder / writer (rp_builder.cpp)
bool compute_wav_mfccs(Ctx *ctx, const uint8_t *buf, size_t len, int K, std::vector<float> *mfcc, int *frames, float *rms_level);
bool build_wakeword_ref(Ctx *ctx, const std::string &name, const float *threshold, const float *avg_threshold, size_t n,
                        const char *const *sample_names, const uint8_t *const *wavs, const size_t *wav_lens, int mfcc_size,
                        bool rms_median, WakewordRefData *out);
// the batched forms: MfccAverager::average for W wakewords (HOST arrays: counts [W], lens [sum counts] in fold order, feats [sum lens][K];
// avg: lens[first template of w] rows per wakeword), and build_wakeword_ref for W wakewords with one MFCC launch, the normalisation and
// the averaging on the device (rp_average.hip)
bool average_templates_batch(Ctx *ctx, size_t W, int K, const int32_t *counts, const int32_t *lens, const float *feats, float *avg);
bool build_wakeword_refs(Ctx *ctx, size_t W, const char *const *names, const float *thresholds, const float *avg_thresholds,
                         const size_t *counts, const char *const *sample_names, const uint8_t *const *wavs, const size_t *wav_lens,
                         int mfcc_size, bool rms_median, std::vector<WakewordRefData> *out);
// build_wakeword_refs in two parts.  enrol_front: everything up to and including the fold -- the call's templates (fold order) and averages
// lie in ctx->ws_enrol, [rows][K] | [avg_rows][K], and `refs` holds what the host knows of every wakeword (name, thresholds, template names
// and lengths in file order, rms_level, has_avg / avg_len; no features).  enrol_fetch: the copy back that fills the features in.
struct EnrolSample { std::vector<float> mono; const struct Resampler *rs = nullptr; size_t enc_chunk = 480; int frames = 0; float level = 0.f; bool live = true; int64_t dst_row = 0; };
struct EnrolBatch {
    std::vector<WakewordRefData> refs;
    std::vector<EnrolSample> smp;                    // dst_row: a sample's first row among the templates
    std::vector<std::vector<size_t>> slot_sample;    // per wakeword and template slot (file order) its sample
    size_t rows = 0, avg_rows = 0;
    std::vector<int64_t> avg_row;                    // per wakeword the first row of its average among the averages, -1: none
};
bool enrol_front(Ctx *ctx, size_t W, const char *const *names, const float *thresholds, const float *avg_thresholds,
                 const size_t *counts, const char *const *sample_names, const uint8_t *const *wavs, const size_t *wav_lens,
                 int mfcc_size, bool rms_median, size_t first_index, EnrolBatch *out);
bool enrol_fetch(Ctx *ctx, int K, EnrolBatch *b);
std::vector<uint8_t> serialize_wakeword_ref(const WakewordRefData &r);
std::vector<std::vector<uint8_t>> serialize_wakeword_refs(const std::vector<WakewordRefData> &refs);   // the same, on several host threads
std::vector<uint8_t> serialize_wakeword_model(const WakewordModelData &m);
// trainer (rp_train.cpp)
bool model_dims(int m_type, size_t input_len, int mfcc_size, size_t n_labels, std::vector<int> *dims);
bool train_wakeword_model(Ctx *ctx, const rp_train_options &opt, size_t n_train, const char *const *train_names,
                          const uint8_t *const *train_wavs, const size_t *train_lens, size_t n_test, const char *const *test_names,
                          const uint8_t *const *test_wavs, const size_t *test_lens, const WakewordModelData *prev,
                          WakewordModelData *out, float *final_loss, float *test_accuracy);
// train_wakeword_model for W models in one call: the samples of all models follow each other (train_counts / test_counts [W]); seeds [W]
// (null: opt.seed + w); prev [W] (null or an entry null: none).  The epochs of all models run in train_batch_kernel.  A model the single
// call refuses fails the call with that error behind "model <index>: ".
bool train_wakeword_models(Ctx *ctx, const rp_train_options &opt, size_t W, const uint64_t *seeds, const size_t *train_counts,
                           const char *const *train_names, const uint8_t *const *train_wavs, const size_t *train_lens,
                           const size_t *test_counts, const char *const *test_names, const uint8_t *const *test_wavs, const size_t *test_lens,
                           const WakewordModelData *const *prev, std::vector<WakewordModelData> *out, float *final_loss, float *test_accuracy,
                           size_t first_index = 0, struct TrainLeft *left = nullptr);
// What a training call leaves on the device for a caller that goes on there (rp_model_bank_train): the trained layer l of model w lies at
// ctx->ws_train + jobs[w].w[l] / jobs[w].b[l] (floats, 16-byte aligned) until the next call that uses the workspace.  first_index: the
// index a refusal names model 0 of the call by.
struct TrainLeft { std::vector<TrainJob> jobs; };
// The epochs alone: one MLP per item, HOST arrays.  params in / out: per layer, weight [out][in] then bias [out]; loss_rows [B] (null: not
// wanted): the rows of the last epoch's loss; tlog [Bt][dims[n_layers]] (null: no test forward): the logits of the test rows xt under the
// final weights.  One upload and one download on the context's stream; launches of at most E epochs (rp_train.cpp).
struct MlpTrainItem {
    int n_layers = 0;
    int dims[kTrainMaxLayers + 1] = {0, 0, 0, 0, 0};
    size_t B = 0, Bt = 0;
    const float *x = nullptr, *xt = nullptr;
    const int32_t *labels = nullptr;
    float *params = nullptr, *loss_rows = nullptr, *tlog = nullptr;
};
bool train_mlp_batch(Ctx *ctx, const std::vector<MlpTrainItem> &items, float learning_rate, size_t epochs, TrainLeft *left = nullptr);

// The host's share of a batch (wav decoding, levels, weight draws, CBOR) is independent per sample / per wakeword / per model: up to 16 threads take indices from
// one counter.  The first exception of a worker is rethrown on the calling thread.
template <class F> void parallel_for(size_t n, F &&f) {
    const size_t nt = std::min<size_t>({(size_t)16, (size_t)std::max(1u, std::thread::hardware_concurrency()), n / 4});
    if (nt <= 1) { for (size_t i = 0; i < n; ++i) f(i); return; }
    std::atomic<size_t> next{0};
    std::atomic<bool> failed{false};
    std::exception_ptr error;
    auto work = [&] {
        try {
            for (size_t i; !failed.load() && (i = next.fetch_add(1)) < n;) f(i);
        } catch (...) {
            if (!failed.exchange(true)) error = std::current_exception();
        }
    };
    std::vector<std::thread> pool;
    try {
        for (size_t t = 1; t < nt; ++t) pool.emplace_back(work);
    } catch (...) {}   // fewer threads than asked for: the others take the work
    work();
    for (std::thread &t : pool) t.join();
    if (error) std::rethrow_exception(error);
}

void set_last_error(const std::string &msg);
const std::string &last_error();
bool hip_ok(hipError_t e, const char *what);

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    ~DevBuf();
    bool reserve(size_t bytes);  // grows, contents NOT preserved
    template <class T> T *as() const { return static_cast<T *>(p); }
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
};

// page-locked host memory the device reads / writes in place (the single-stream path's chunk and results)
struct PinBuf {
    void *p = nullptr;      // host pointer
    void *dev = nullptr;    // the same memory as the device sees it
    size_t cap = 0;
    ~PinBuf();
    bool reserve(size_t bytes);  // grows, contents NOT preserved
    template <class T> T *as() const { return static_cast<T *>(p); }
    template <class T> T *dev_as() const { return static_cast<T *>(dev); }
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
};

struct Ctx {
    int device = 0;
    int flags = 0;
    DtwArith arith;   // the DTW launchers' arithmetic (RP_CTX_ARITH_* at creation, rp_ctx_set_arithmetic); every template set of the context points here
    int n_cu = 256;  // compute units of the device (persistent kernels launch one workgroup per CU)
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::map<int, MfccTablesDev> tables;  // by K
    std::map<size_t, std::unique_ptr<struct Resampler>> resamplers;  // by input sample rate
    DevBuf ws_resample;
    // timing
    bool timing = false;
    struct Timed { hipEvent_t a, b; int kernel; };
    std::vector<Timed> pending;
    double sum_ms[kKernelCount] = {0};
    int count[kKernelCount] = {0};
    // staging for RP_CTX_HOST_POINTERS
    DevBuf stage_in, stage_out, stage_out2, stage_out3;
    // intermediates of rp_batch_detect
    DevBuf ws_mfcc, ws_scores, ws_agg, ws_avg, ws_vad, ws_ring, ws_rms, ws_gain, ws_list, ws_hot;
    // floats of ws_scores the last rp_batch_detect* wrote as its [S * n_win][T] score block (rp_ctx_last_window_scores); 0: none, the
    // scores went to the caller's device array, or another call has used the workspace since
    size_t last_window_scores = 0;
    DevBuf ws_bank_idx;  // the per-stream wakeword indices of a bank call with RP_CTX_HOST_POINTERS
    DevBuf ws_gain_tab;  // rp_frontend_batch_bank_sets / _model_bank: the per-stream table of stream_targets_kernel
    DevBuf ws_set_ww, ws_set_agg, ws_set_avg;  // wakeword-set calls: the proposals' bank indices [S][n_win]; the per-slot rows of a call with host pointers
    // mixed-set calls (rp_batch_detect_mixed_sets): the model rows' staged indices and the model side's four proposal rows [S][n_win] -- the
    // reference side's live in ws_bank_idx / ws_agg / ws_avg / ws_set_ww, and both are read by one scan
    DevBuf ws_mix_idx, ws_mix_best, ws_mix_avg, ws_mix_ww, ws_mix_label;
    DevBuf ws_dtw;  // [2 * kDtwSchedChunks | 2 + 2 * kDtwFixCap] uint32: tile counters and fix list of the DTW launchers, zero between calls
    // rp_batch_detect_ingest: copy stream, two device blocks of PCM, per block "copy landed" / "kernels done with it" events
    hipStream_t copy_stream = nullptr;
    hipEvent_t ingest_landed[2] = {nullptr, nullptr}, ingest_freed[2] = {nullptr, nullptr};
    DevBuf ws_ingest;
    bool ingest_ready();   // creates the stream and events on first use
    // per-stream "a window of this stream can fire" flags between the aggregate pass and the scan: zero between calls (the scan clears
    // what it reads; a call that fails in between leaves spurious 1s, which only cost the next scan its shortcut), zeroed here when the
    // buffer grows
    uint32_t *hot_flags(size_t S);
    // the list of rows the wakeword-model forward computes again with the f32 matrix instructions (kMlpF16x2, rp_kernels.h): [2 + B]
    // words, the first two zero between calls
    DevBuf ws_mlp_redo;
    uint32_t *mlp_redo(size_t B);
    std::string last_mlp_kernel;   // what the last dense-row forward ran (rp_ctx_last_mlp_kernel)
    mutable uint32_t dtw_ran = 0;  // kDtwRan* of the DTW launches since rp_ctx_dtw_kernels last read it
    DtwWork dtw_work() const { return DtwWork{ws_dtw.as<uint32_t>(), ws_dtw.as<uint32_t>() + 2 * kDtwSchedChunks, &dtw_ran}; }
    // ... plus the blocks dtw_ragged_kernel needs for a call over S streams x n_win windows (whole-stream batches; a failed reservation
    // only means that kernel is not taken)
    DevBuf ws_rag;
    DtwWork dtw_work_for(size_t S, size_t rows);
    // enrolment batches (rp_builder.cpp): the call's templates and averages; its padded samples, their frame counts, their places among the
    // templates and their raw frames; the averaging kernel's index arrays; the cost matrices of the wakewords whose matrix does not fit the
    // LDS (one slice per workgroup of that launch); page-locked staging (at most 128 MB) the padded samples pass through
    DevBuf ws_enrol, ws_enrol_pcm, ws_enrol_nf, ws_enrol_dst, ws_enrol_raw, ws_enrol_i32, ws_enrol_i64, ws_avg_matrix;
    PinBuf enrol_stage;
    // batched training (rp_train.cpp): the job table and every model's rows, weights and intermediates (TrainJob, rp_kernels.h); what the
    // last call spent (rp_train_batch_last_profile): its feature stage on the host clock and, with timing enabled, its launches
    DevBuf ws_train;
    double train_feature_ms = 0.0, train_longest_launch_ms = 0.0;
    int train_launches = 0;

    static Ctx *create(int device, int flags);
    ~Ctx();
    const MfccTablesDev *tables_for(int K);
    const Resampler *resampler_for(size_t fs_in);  // plans are cached per input rate
    void time_begin(int kernel);
    void time_end();
    void time_collect();
};

// AudioEncoder's resampler (src/audio/encoder.rs:72-83) as a device-resident linear map, rp_resampler.cpp
bool resampler_frame_lengths(size_t fs_in, size_t *in_len, size_t *out_len);
struct Resampler {
    Ctx *ctx = nullptr;
    ResamplerDev dev;
    DevBuf g2t, fft48;
    static Resampler *create(Ctx *ctx, size_t fs_in);
};

// one template row as the DTW kernels read it: unit [K] and raw [K]; see rp_ctx.cpp
bool prepare_template_row(const float *src, int K, float *unit, float *raw, bool *ref_only);

struct Templates {
    Ctx *ctx = nullptr;
    TemplatesDev dev;
    static Templates *create(Ctx *ctx, int T, int K, const int *lens, const float *feats, int avg_len,
                             const float *avg);
    ~Templates();
};

// A wakeword bank (rp_bank.cpp; its calls: rp_bank_calls.cpp): W wakeword references uploaded once, scored per stream through an index (rp_dtw_bank.hip).  Borrows the context.
struct Bank {
    Ctx *ctx = nullptr;
    BankDev dev;
    std::vector<BankWakeword> ww;   // the host's copy of dev.ww
    // WakewordRef::rms_level of every wakeword (NaN: none), beside dev.ww on the device: what the per-stream gain normaliser reads through a
    // stream's index (PerStreamGain)
    std::vector<float> rms_levels;
    float *rms_level = nullptr;     // [W], device
    bool set_rms_levels(const float *levels);   // HOST array [W]; ordered on the context's stream
    // HOST arrays in the flat layout of rp_mfcc_average_batch: counts [W], lens [sum counts], feats [sum lens][K]; avg_lens [W] (0: none) and
    // avg_feats [sum avg_lens][K] (both may be null); thresholds / avg_thresholds [W] (null or NaN: none)
    static Bank *create(Ctx *ctx, size_t W, int K, const int32_t *counts, const int32_t *lens, const float *feats, const int32_t *avg_lens,
                        const float *avg_feats, const float *thresholds, const float *avg_thresholds);
    ~Bank();

    // ---- a bank that grows (rp_wakeword_bank_reserve / _put / _put_from_rpw / _enrol).  The five device arrays and rms_level are pools:
    // new entries and rows are appended behind n_entries / n_rows, a replaced wakeword's old ones stay behind as garbage (dead_*), and a full
    // pool is replaced by a larger one into which only the live entries and rows move (bank_move_kernel).  Everything is enqueued on the
    // context's stream, so a launch that took the old BankDev by value finishes on the old pools before they are freed.
    std::vector<int> tlen;          // the host's copy of dev.tlen / dev.trow, [n_entries]
    std::vector<long long> trow;
    size_t n_entries = 0, n_rows = 0, dead_entries = 0, dead_rows = 0;
    size_t cap_ww = 0, cap_entries = 0, cap_rows = 0;
    size_t grown = 0;               // how often the entry / row pools were replaced (tests)
    int ceiling = 0;                // rp_wakeword_bank_reserve: no wakeword's window may be longer (0: none)
    mutable int live_batches = 0;   // stream batches over this bank (rp_stream_batch_new_bank .. _free)
    DevBuf put_ws;                  // index tables and flags of a put / a move
    // one wakeword of a put: its sample templates in the wakeword's own order (frames, first row in the source), its averaged template
    struct PutItem {
        std::vector<int> lens;
        std::vector<long long> src;
        int avg_len = 0;
        long long avg_src = 0;
        float threshold = NAN, avg_threshold = NAN, rms_level = NAN;
        int max_len() const { int m = 0; for (int l : lens) m = l > m ? l : m; return m; }
    };
    // what Bank::create checks in a wakeword, for wakewords first .. first + items.size() - 1, and `first` itself; changes nothing
    bool put_check(size_t first, const std::vector<PutItem> &items) const;
    // d_src: DEVICE rows [..][K] the items' src point into.  Prepares the rows in the pool tail (bank_put_kernel), reads the kernel's
    // verdict, and only then commits ww[] / rms_level; returns after the stream has drained.  A refusal leaves the bank as it was.
    bool put_rows(size_t first, const std::vector<PutItem> &items, const float *d_src);
    bool reserve(int max_len, size_t n_wakewords, size_t rows);
    bool grow_ww(size_t cap);                           // dev.ww / rms_level with room for `cap` wakewords
    bool repool(size_t entries_cap, size_t rows_cap);   // new entry and row pools of these capacities, the live entries moved over
    int max_window() const { return std::max(std::max(ceiling, dev.max_len), 1); }   // what a stream batch over the bank keeps room for
};

struct Model {
    Ctx *ctx = nullptr;
    MlpDev dev;
    bool mfma_ok = false;  // layer-1 shape supported by the MFMA kernels
    std::vector<float *> W, B;  // plain per-layer device copies for the generic kernel
    std::vector<int> dims;
    std::vector<float> w1_host;                     // layer-1 weights [dims[1]][dims[0]]
    std::map<int, std::unique_ptr<DevBuf>> wsums;   // per mfcc_size K: [16*nt][K], sum over frames of the layer-1 weights
    const float *wsum_for(int K);                   // (takes the window mean out after layer 1, MlpForward::windows)
    std::unique_ptr<DevBuf> stream_img[6];          // per precision (kMlpF32 / kMlpBf16 / kMlpF16x2 / kMlpBf16x3): layer-1 weights in the stream kernel's fragment order
    int stream_ksteps = 0;                          // k-steps of 32 the images hold (zero padded past dims[0])
    // plan of launch_mlp_stream for rows starting at x (x decides the phases), for a call mlp_stream_supported admits
    bool stream_plan(const float *x, size_t B, int precision, MlpStreamPlan *plan);
    // weights/biases: HOST arrays, W_l [dims[l+1]][dims[l]], b_l [dims[l+1]]
    static Model *create(Ctx *ctx, int n_layers, const int *dims, const float *const *weights, const float *const *biases);
    ~Model();
};

// init_model of a parsed wakeword model (src/wakewords/nn/wakeword_nn.rs:165-389, "Incorrect model layers" :252-256): its layers by type
// (Tiny: ln1, ln2; the others ln1..ln3), the tensors checked against their declared shapes, the index of the "none" label (-1: none).
// nullptr with the error set.  (rp_model_bank.cpp; the single-stream detector and the model bank load .rpw models through it)
Model *model_from_data(Ctx *ctx, const WakewordModelData &model, int *n_layers, std::vector<int> *dims, int *none_index);

// A model bank (rp_model_bank.cpp; its calls: rp_bank_calls.cpp): W wakeword models copied into pools on the device, run per stream through an index
// (mlp_windows_bank_kernel in rp_mlp_windows.hip).  Borrows the context.
struct ModelBank {
    Ctx *ctx = nullptr;
    ModelBankDev dev;                // label_pitch: max(res_labels, the largest label count)
    std::vector<ModelBankEntry> e;   // the host's copy of dev.e
    DevBuf d_e, d_wimg, d_b1, d_wsum, d_tail, d_ww;
    BankDev scan;                    // W and a BankWakeword per model for scan_bank_kernel: max_len = L, avg set, both thresholds -1
    int max_L = 0, min_L = 0;
    // WakewordModel::rms_level of every model (NaN: none), beside scan.ww on the device: what the gain normaliser of a stream reads through
    // its indices (GainSource), as Bank::rms_levels / rms_level
    std::vector<float> rms_levels;
    DevBuf d_level;                  // [cap_models], device
    const float *rms_level() const { return d_level.as<float>(); }
    bool set_rms_levels(const float *levels);   // HOST array [W]; ordered on the context's stream
    // models: W handles of this context; none_index [W] (null: every -1); levels [W] (null: every NaN); false with the error set
    static ModelBank *create(Ctx *ctx, size_t W, Model *const *models, int mfcc_size, const int32_t *none_index, const float *levels = nullptr);

    // ---- a bank that grows (rp_model_bank_reserve / _put / _put_from_rpw / _train), after Bank's.  The six device arrays are pools: a put
    // appends its entries behind used[] (model_bank_put_kernel builds them there), a replaced model's old ones stay behind as garbage
    // (dead[]), and a full pool is replaced by one of at least twice the size into which only the live models move
    // (model_bank_move_kernel).  Everything is enqueued on the context's stream, so a launch that took the old ModelBankDev by value finishes
    // on the old pools before they are freed.
    enum { kImg = 0, kB1 = 1, kWsum = 2, kTail = 3 };   // wimg counts 16-byte pieces, the others floats
    size_t used[4] = {0, 0, 0, 0}, dead[4] = {0, 0, 0, 0}, cap[4] = {0, 0, 0, 0};
    size_t cap_models = 0;           // rows d_e / d_ww have room for
    size_t grown = 0;                // how often the four pools were replaced (tests)
    int res_L = 0, res_labels = 0;   // rp_model_bank_reserve: no model's window / label count may be larger (0: none)
    mutable int live_batches = 0;    // stream batches over this bank (rp_stream_batch_new_model_bank .. _free)
    DevBuf put_ws;                   // item table and flags of a put, entry tables of a move
    // one model of a put: its raw parameters on the DEVICE and its shape (entry: everything but the four pool places)
    struct PutItem {
        const float *w[3] = {nullptr, nullptr, nullptr}, *b[3] = {nullptr, nullptr, nullptr};
        ModelBankEntry entry{};
        float rms_level = NAN;
    };
    // What the bank refuses in a model of these layer widths, as ModelBank::create words it (`why` without the "model <index>: "), and its
    // entry's shape.  image_ok: the handle's verdict on its three-part image; -1: worked out from the shape, as Model::create does.
    static bool entry_of(const std::vector<int> &dims, int none_index, int image_ok, ModelBankEntry *e, std::string *why);
    // `first` itself and what a reservation or a live batch adds to entry_of, for models first .. first + items.size() - 1; `who`: "model" or
    // "wakeword".  Changes nothing.
    bool put_check(size_t first, const std::vector<PutItem> &items, const char *who) const;
    // Builds the entries in the pool tails, reads the kernel's verdict and only then commits the descriptors; returns after the stream has
    // drained.  A refusal leaves the bank as it was.
    bool put(size_t first, const std::vector<PutItem> &items, const char *who);
    bool reserve(int max_train_size, int max_labels, size_t n_models, size_t n_frames);
    bool grow_models(size_t n);                    // d_e / d_ww with room for n models
    bool repool(const size_t want[4]);             // new pools of these capacities, the live models moved over
    int max_window() const { return std::max(std::max(res_L, max_L), 1); }   // what a stream batch over the bank keeps room for
    double last_put_ms = 0.0;                      // with rp_ctx_timing_enable: model_bank_put_kernel's time in the last put
};
// The layers of a parsed wakeword model as model_from_data checks them: layer count by type, widths, the tensors (pointers into `model`),
// the index of the "none" label.  False with the error set.
bool model_layers(const WakewordModelData &model, int *n_layers, std::vector<int> *dims, std::vector<const float *> *weights,
                  std::vector<const float *> *biases, int *none_index);

// ------------------------------------------------------------ `Rustpotter` mirror
struct Detection {  // src/detector.rs:488-501
    std::string name;
    float avg_score = 0.f, score = 0.f;
    std::vector<std::string> score_names;
    std::vector<float> scores;
    size_t counter = 0;
    float gain = 0.f;
};

class Rustpotter {
public:
    static Rustpotter *create(const rp_config &cfg);
    ~Rustpotter();
    bool add_wakeword_from_buffer(const std::string &key, const uint8_t *buf, size_t len);
    bool add_wakeword_from_file(const std::string &key, const std::string &path);
    bool remove_wakeword(const std::string &key);
    bool remove_wakewords();
    size_t get_samples_per_frame() const { return in_len_ * (size_t)fmt_.channels; }  // AudioEncoder::get_input_frame_length
    size_t get_bytes_per_frame() const;
    const Detection *get_partial_detection() const { return has_partial_ ? &partial_ : nullptr; }
    float get_rms_level() const { return rms_level_; }
    float get_gain() const { return gain_; }
    float get_rms_level_ref() const;
    // returns 1 detection, 0 none, <0 error
    int process_bytes(const uint8_t *bytes, size_t len, Detection *out);
    template <class T> int process_samples(const T *samples, size_t n, Detection *out);
    void update_detector_config(const rp_detector_config &c);
    void update_filters_config(const rp_filters_config &c);
    void reset();

private:
    Rustpotter() = default;
    int encode_and_process(float *mono, Detection *out);   // resample (if any) -> process_audio
    int process_audio(float *buf, size_t n, Detection *out);
    void on_wakeword_change();
    bool add_wakeword_ref(const std::string &key, WakewordRefData &&ref);
    bool add_wakeword_model(const std::string &key, WakewordModelData &&model);
    bool prepare_first(int K);
    bool run_detection(int frame_slot, Detection *out);

    struct Wakeword;
    bool gate_first_ = false;   // process_audio: score the averaged template before the others (the gate rejected the last chunk)
    std::unique_ptr<Ctx> ctx_;
    rp_audio_fmt fmt_{};
    rp_detector_config det_{};
    rp_filters_config filt_{};
    std::vector<std::pair<std::string, std::unique_ptr<Wakeword>>> wakewords_;  // insertion order
    int K_ = 0;
    // AudioEncoder (src/audio/encoder.rs): frame lengths and, for input that is not 16 kHz, the resampler
    // plan with the previous input frame kept on the device
    size_t in_len_ = 480, out_len_ = 480;
    const Resampler *rs_ = nullptr;
    PinBuf rs_x_, enc_;          // [2*in_len] previous | current input frame, [out_len] the encoded (16 kHz) chunk:
                                 // page-locked host memory the resampler kernel reads / writes in place
    // extractor state (src/mfcc/extractor.rs:14, :66-79): the last two 10 ms shifts and how many are buffered
    size_t shifts_seen_ = 0;     // capped at 3: a frame is emitted from the 4th shift on
    PinBuf up_;                  // [160 pad | 2 buffered shifts | new shifts]: the MFCC kernel reads it in place
    // audio_mfcc_window (src/detector.rs:69): device history + explicit length
    DevBuf hist_;                // [hist_cap][K]
    size_t hist_cap_ = 0, n_hist_ = 0, win_len_ = 0, max_mfcc_frames_ = 0;
    DevBuf nn_x_, nn_s0_, nn_s1_;
    PinBuf result_;              // [frames | per wakeword score blocks]: written by the kernels, read by the host
    // detection state (src/detector.rs:71-79)
    bool has_partial_ = false;
    Detection partial_;
    size_t countdown_ = 0;
    float rms_level_ = 0.f, gain_ = 1.f;
    // VAD (src/mfcc/vad.rs)
    struct Vad { float mode_value = 2.f; size_t index = 0; float window[50]; size_t voice_countdown = 0; void reset(); bool is_voice(const float *mfcc, int K); };
    bool has_vad_ = false;
    Vad vad_;
    // filters (src/audio/gain_normalizer_filter.rs, band_pass_filter.rs)
    struct Gain { bool enabled = false, fixed = false; size_t window_size = 1; float min_gain = 0.1f, max_gain = 1.f, rms_level_ref = 0.f, rms_level_sqrt = 0.f; std::vector<float> win; };
    struct BandPass { bool enabled = false; float a0, a1, a2, b1, b2, x1, x2, y1, y2; };
    Gain gainf_;
    BandPass bp_;
    void configure_filters();
};

}  // namespace rp
