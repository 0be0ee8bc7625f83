// rp_train.cpp -- WakewordModelTrain::train_from_buffers (src/wakewords/nn/wakeword_model_train.rs:44-168) on the
// device: MFCC features of labelled wav samples (MFCC kernel, resampler for wavs that are not 16 kHz), the
// reference's MLP shapes (wakeword_nn.rs:305-389), full-batch log-softmax / nll / SGD epochs, and the result as a
// WakewordModel .rpw (wakeword_model.rs:11-18).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "rp_host.h"

namespace rp {

namespace {
// label = lower-cased text between the first '[' and the first ']' of the file name, "none" without one (:283-295)
std::string label_of(const std::string &name) {
    // the reference works on chars; the names it is used with are ASCII around the brackets
    const size_t a = name.find('['), b = name.find(']');
    if (a == std::string::npos || b == std::string::npos || !(a < b)) return "none";
    std::string l = name.substr(a + 1, b - a - 1);
    for (char &c : l) c = (char)std::tolower((unsigned char)c);
    return l;
}

struct Rng {  // seeded generator for a fresh model's weights (the reference draws from the thread RNG: never reproducible)
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double uni() { return ((double)(next() >> 11) + 0.5) / 9007199254740992.0; }  // (0,1)
    double normal() { const double u = uni(), v = uni(); return std::sqrt(-2.0 * std::log(u)) * std::cos(2.0 * M_PI * v); }
};

struct Sample { std::vector<float> feat; int label; };

// get_mfccs_labeled, :274-325
bool labelled_features(Ctx *ctx, size_t n, const char *const *names, const uint8_t *const *wavs, const size_t *lens, int K,
                       std::vector<std::string> *labels, bool new_labels, float *rms_level, std::vector<Sample> *out) {
    for (size_t i = 0; i < n; ++i) {
        const std::string label = label_of(names[i]);
        auto it = std::find(labels->begin(), labels->end(), label);
        if (it == labels->end()) {
            if (!new_labels) {
                set_last_error("Forbidden label '" + label + "', it doesn't exists on the training data or in the model you are training from.");
                return false;
            }
            labels->push_back(label);
            it = labels->end() - 1;
        }
        Sample s;
        s.label = (int)(it - labels->begin());
        int frames = 0; float level = 0.f;
        if (!compute_wav_mfccs(ctx, wavs[i], lens[i], K, &s.feat, &frames, &level)) return false;
        if (rms_level && label != "none") *rms_level = std::isnan(*rms_level) ? level : (*rms_level + level) / 2.f;
        out->push_back(std::move(s));
    }
    return true;
}
}  // namespace

// the layer widths of Tiny / Small / Medium / Large, wakeword_nn.rs:305-389 (MFCCS_EXTRACTOR_OUT_SHIFTS = 3)
bool model_dims(int m_type, size_t input_len, int mfcc_size, size_t n_labels, std::vector<int> *dims) {
    const size_t fr = input_len / (size_t)mfcc_size;
    dims->clear();
    dims->push_back((int)input_len);
    switch (m_type) {
    case 0: dims->push_back((int)(fr / 15)); break;
    case 1: dims->push_back((int)(fr / 6)); dims->push_back((int)((fr / 6) / 2)); break;
    case 2: dims->push_back((int)(fr / 3)); dims->push_back((int)(fr / 6)); break;
    case 3: dims->push_back((int)((fr / 3) * 2)); dims->push_back((int)(fr / 6)); break;
    default: set_last_error("unknown model type"); return false;
    }
    dims->push_back((int)n_labels);
    for (size_t i = 1; i + 1 < dims->size(); ++i)
        if ((*dims)[i] < 1) { set_last_error("training samples too short for this model type"); return false; }
    return true;
}

static const char *kTypeNames[4] = {"Tiny", "Small", "Medium", "Large"};

namespace {
// One model between the three parts of a training: prepare (labels, features, rms level, shapes, the weights to start from), the epochs
// (launch_train_step for one model, train_batch_kernel for many) and finish (loss, test accuracy, the WakewordModel).
struct Prepared {
    std::vector<std::string> labels;
    int m_type = 0, K = 0;
    float rms_level = NAN;
    size_t input_len = 0;
    std::vector<int> dims;
    bool seeded = false;                  // the weights are still to be drawn (prepare_rows)
    uint64_t seed = 0;
    std::vector<Sample> train, test;      // until prepare_rows
    std::vector<float> params;            // per layer, weight [out][in] then bias [out]
    std::vector<float> xtr, xte;          // [B][input_len], [Bt][input_len]
    std::vector<int32_t> ytr, yte;
    std::vector<float> loss_rows, tlog;   // what the epochs leave: [B] of the last epoch, [Bt][labels] of the final weights
    int n_layers() const { return (int)dims.size() - 1; }
    size_t w_off(int l) const { size_t o = 0; for (int i = 0; i < l; ++i) o += ((size_t)dims[i] + 1) * (size_t)dims[i + 1]; return o; }
    size_t b_off(int l) const { return w_off(l) + (size_t)dims[l] * (size_t)dims[l + 1]; }
};

// prepare, the part that can refuse and that uses the context: everything of train_from_buffers up to the weights (:44-112)
bool prepare_model(Ctx *ctx, const rp_train_options &opt, size_t n_train, const char *const *train_names, const uint8_t *const *train_wavs,
                   const size_t *train_lens, size_t n_test, const char *const *test_names, const uint8_t *const *test_wavs,
                   const size_t *test_lens, const WakewordModelData *prev, Prepared *p) {
    if (n_train == 0) { set_last_error("No training data provided"); return false; }
    if (n_test == 0) { set_last_error("No test data provided"); return false; }
    p->m_type = opt.m_type; p->K = (int)opt.mfcc_size; p->seed = opt.seed;
    if (prev) {  // "Training from previous model, some options will be ignored."
        p->labels = prev->labels;
        p->K = prev->mfcc_size;
        p->m_type = -1;
        for (int t = 0; t < 4; ++t) if (prev->m_type == kTypeNames[t]) p->m_type = t;
        if (p->m_type < 0) { set_last_error("unknown model type in the model to train from"); return false; }
    }
    const int K = p->K;
    if (K < 1) { set_last_error("mfcc_size must be >= 1"); return false; }
    if (!labelled_features(ctx, n_train, train_names, train_wavs, train_lens, K, &p->labels, prev == nullptr, &p->rms_level, &p->train)) return false;
    if (!labelled_features(ctx, n_test, test_names, test_wavs, test_lens, K, &p->labels, false, nullptr, &p->test)) return false;
    if (p->labels.size() < 2) { set_last_error("Your training data need to contain at least two labels"); return false; }
    size_t input_len = 0;
    if (prev) input_len = prev->train_size * (size_t)K;
    else for (const Sample &s : p->train) input_len = std::max(input_len, s.feat.size());
    if (input_len == 0) { set_last_error("training samples too short"); return false; }
    p->input_len = input_len;
    if (!model_dims(p->m_type, input_len, K, p->labels.size(), &p->dims)) return false;
    const int nl = p->n_layers();
    p->params.resize(p->w_off(nl));
    p->seeded = prev == nullptr;
    if (prev) {
        for (int l = 0; l < nl; ++l) {
            const size_t in = (size_t)p->dims[l], on = (size_t)p->dims[l + 1];
            const std::string wn = "ln" + std::to_string(l + 1) + ".weight", bn = "ln" + std::to_string(l + 1) + ".bias";
            auto wi = prev->weights.find(wn), bi = prev->weights.find(bn);
            if (wi == prev->weights.end() || bi == prev->weights.end() || wi->second.second.size() != in * on || bi->second.second.size() != on) {
                set_last_error("Incorrect model layers");
                return false;
            }
            std::memcpy(p->params.data() + p->w_off(l), wi->second.second.data(), in * on * sizeof(float));
            std::memcpy(p->params.data() + p->b_off(l), bi->second.second.data(), on * sizeof(float));
        }
    }
    return true;
}

// prepare, the part that is the model's own and cannot fail: a fresh model's weights -- candle_nn::linear's initialisation (weights
// N(0, sqrt(2/fan_in)), biases U(-1/sqrt(fan_in), 1/sqrt(fan_in))) from a seeded generator -- and the rows, padded / truncated to
// input_len (:113-116)
void prepare_rows(Prepared *p) {
    const int nl = p->n_layers();
    if (p->seeded) {
        Rng rng{p->seed};
        for (int l = 0; l < nl; ++l) {
            const size_t in = (size_t)p->dims[l], on = (size_t)p->dims[l + 1];
            const double std_w = std::sqrt(2.0) / std::sqrt((double)in), bound = 1.0 / std::sqrt((double)in);
            float *w = p->params.data() + p->w_off(l), *b = p->params.data() + p->b_off(l);
            for (size_t i = 0; i < in * on; ++i) w[i] = (float)(rng.normal() * std_w);
            for (size_t i = 0; i < on; ++i) b[i] = (float)((rng.uni() * 2.0 - 1.0) * bound);
        }
    }
    const size_t input_len = p->input_len;
    auto pack = [&](std::vector<Sample> &set, std::vector<float> *x, std::vector<int32_t> *y) {
        x->assign(set.size() * input_len, 0.f); y->resize(set.size());
        for (size_t i = 0; i < set.size(); ++i) {
            std::memcpy(x->data() + i * input_len, set[i].feat.data(), std::min(set[i].feat.size(), input_len) * sizeof(float));
            (*y)[i] = set[i].label;
        }
        std::vector<Sample>().swap(set);
    };
    pack(p->train, &p->xtr, &p->ytr); pack(p->test, &p->xte, &p->yte);
    p->loss_rows.assign(p->ytr.size(), 0.f);
    p->tlog.assign(p->yte.size() * p->labels.size(), 0.f);
}

// finish: the last epoch's loss (computed before its update, like candle's loss value), summed over the rows in order; the test accuracy of
// the final weights (test_model :251-272: argmax, first maximum, == label); the WakewordModel
void finish_model(Prepared &p, size_t epochs, WakewordModelData *out, float *final_loss, float *test_accuracy) {
    const size_t B = p.ytr.size(), Bt = p.yte.size(), C = p.labels.size();
    if (final_loss) { float s = 0.f; for (float v : p.loss_rows) s += v; *final_loss = epochs ? s / (float)B : NAN; }
    if (test_accuracy) {
        size_t ok = 0;
        for (size_t b = 0; b < Bt; ++b) {
            size_t best = 0;
            for (size_t c = 1; c < C; ++c) if (p.tlog[b * C + c] > p.tlog[b * C + best]) best = c;
            ok += (int)best == p.yte[b] ? 1 : 0;
        }
        *test_accuracy = (float)ok / (float)Bt;
    }
    WakewordModelData m;
    m.labels = p.labels; m.train_size = p.input_len / (size_t)p.K; m.mfcc_size = p.K; m.m_type = kTypeNames[p.m_type]; m.rms_level = p.rms_level;
    for (int l = 0; l < p.n_layers(); ++l) {
        const size_t in = (size_t)p.dims[l], on = (size_t)p.dims[l + 1];
        const float *w = p.params.data() + p.w_off(l), *b = p.params.data() + p.b_off(l);
        m.weights["ln" + std::to_string(l + 1) + ".weight"] = {{on, in}, std::vector<float>(w, w + in * on)};
        m.weights["ln" + std::to_string(l + 1) + ".bias"] = {{on}, std::vector<float>(b, b + on)};
    }
    *out = std::move(m);
}

// the epochs of ONE model: launch_train_step per epoch, the test forward, the copies back (training_loop :170-222)
bool train_epochs_single(Ctx *ctx, Prepared &p, float learning_rate, size_t epochs) {
    const int nl = p.n_layers();
    const std::vector<int> &dims = p.dims;
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return false;
    hipStream_t st = ctx->stream;
    const size_t B = p.ytr.size(), Bt = p.yte.size(), Bmax = std::max(B, Bt);
    DevBuf dx, dxt, dy, dloss;
    if (!dx.reserve(p.xtr.size() * 4) || !dxt.reserve(p.xte.size() * 4) || !dy.reserve(B * 4) || !dloss.reserve(B * 4)) return false;
    std::vector<DevBuf> dW((size_t)nl), dB((size_t)nl), dact((size_t)nl), ddz((size_t)nl);
    std::vector<float *> pW, pB, pact, pdz;
    for (int l = 0; l < nl; ++l) {
        const size_t nw = (size_t)dims[l] * (size_t)dims[l + 1], nb = (size_t)dims[l + 1];
        if (!dW[l].reserve(nw * 4) || !dB[l].reserve(nb * 4) || !dact[l].reserve(Bmax * (size_t)dims[l + 1] * 4) ||
            !ddz[l].reserve(Bmax * (size_t)dims[l + 1] * 4)) return false;
        if (!hip_ok(hipMemcpyAsync(dW[l].p, p.params.data() + p.w_off(l), nw * 4, hipMemcpyHostToDevice, st), "hipMemcpyAsync") ||
            !hip_ok(hipMemcpyAsync(dB[l].p, p.params.data() + p.b_off(l), nb * 4, hipMemcpyHostToDevice, st), "hipMemcpyAsync")) return false;
        pW.push_back(dW[l].as<float>()); pB.push_back(dB[l].as<float>()); pact.push_back(dact[l].as<float>()); pdz.push_back(ddz[l].as<float>());
    }
    if (!hip_ok(hipMemcpyAsync(dx.p, p.xtr.data(), p.xtr.size() * 4, hipMemcpyHostToDevice, st), "hipMemcpyAsync") ||
        !hip_ok(hipMemcpyAsync(dxt.p, p.xte.data(), p.xte.size() * 4, hipMemcpyHostToDevice, st), "hipMemcpyAsync") ||
        !hip_ok(hipMemcpyAsync(dy.p, p.ytr.data(), B * 4, hipMemcpyHostToDevice, st), "hipMemcpyAsync")) return false;
    for (size_t epoch = 1; epoch <= epochs; ++epoch)
        if (!hip_ok(launch_train_step(st, dx.as<float>(), dy.as<int32_t>(), B, nl, dims.data(), pW.data(), pB.data(), pact.data(), pdz.data(),
                                      learning_rate, dloss.as<float>()), "training step")) return false;
    if (epochs && !hip_ok(hipMemcpyAsync(p.loss_rows.data(), dloss.p, B * 4, hipMemcpyDeviceToHost, st), "hipMemcpyAsync")) return false;
    if (!hip_ok(launch_train_forward(st, dxt.as<float>(), Bt, nl, dims.data(), pW.data(), pB.data(), pact.data()), "test forward")) return false;
    if (!hip_ok(hipMemcpyAsync(p.tlog.data(), pact[nl - 1], p.tlog.size() * 4, hipMemcpyDeviceToHost, st), "hipMemcpyAsync")) return false;
    for (int l = 0; l < nl; ++l)
        if (!hip_ok(hipMemcpyAsync(p.params.data() + p.w_off(l), dW[l].p, (size_t)dims[l] * (size_t)dims[l + 1] * 4, hipMemcpyDeviceToHost, st), "hipMemcpyAsync") ||
            !hip_ok(hipMemcpyAsync(p.params.data() + p.b_off(l), dB[l].p, (size_t)dims[l + 1] * 4, hipMemcpyDeviceToHost, st), "hipMemcpyAsync")) return false;
    return hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize");
}
}  // namespace

bool train_wakeword_model(Ctx *ctx, const rp_train_options &opt, size_t n_train, const char *const *train_names,
                          const uint8_t *const *train_wavs, const size_t *train_lens, size_t n_test, const char *const *test_names,
                          const uint8_t *const *test_wavs, const size_t *test_lens, const WakewordModelData *prev,
                          WakewordModelData *out, float *final_loss, float *test_accuracy) {
    Prepared p;
    if (!prepare_model(ctx, opt, n_train, train_names, train_wavs, train_lens, n_test, test_names, test_wavs, test_lens, prev, &p)) return false;
    prepare_rows(&p);
    if (!train_epochs_single(ctx, p, opt.learning_rate, opt.epochs)) return false;
    finish_model(p, opt.epochs, out, final_loss, test_accuracy);
    return true;
}

// ------------------------------------------------------------------ many models per call
namespace {
// The epoch cut.  No launch may run longer the more epochs a call asks for, so the epochs are cut into launches of at most E; the state
// lies in the workspace between launches, so the cut changes no bit.  E comes from a work estimate: a workgroup's time per epoch is taken
// as the number of multiply-add steps its busiest thread runs one after the other -- per layer the forward's ceil(B*out / T) chains of
// `in` steps, the backprop's ceil(B*in / T) chains of `out` and the update's ceil(ceil(out/4)*(in+1) / T) chains of B, T =
// kTrainBatchThreads -- summed over the jobs the workgroup walks; E = kTrainStepsPerLaunch / the largest such sum, at least 1.  A step
// with its loads took about 30 ns where it was measured (tools/bench_train_batch.py): 2^20 steps are some 30 ms.
// RP_TRAIN_EPOCHS_PER_LAUNCH (read per call, >= 1) replaces E.
constexpr double kTrainStepsPerLaunch = 1048576.0;
constexpr size_t kTrainMaxEpochsPerLaunch = 1u << 20;

double epoch_steps(const MlpTrainItem &it) {
    const double T = (double)kTrainBatchThreads, B = (double)it.B;
    double s = 0.0;
    for (int l = 0; l < it.n_layers; ++l) {
        const double in = it.dims[l], on = it.dims[l + 1];
        s += std::ceil(B * on / T) * in;
        if (l > 0) s += std::ceil(B * in / T) * on;
        s += std::ceil(std::ceil(on / 4.0) * (in + 1.0) / T) * B;
    }
    return s;
}

size_t epochs_per_launch(const std::vector<MlpTrainItem> &items, size_t grid) {
    if (const char *e = std::getenv("RP_TRAIN_EPOCHS_PER_LAUNCH")) {
        char *end = nullptr;
        const unsigned long long v = std::strtoull(e, &end, 10);
        if (end != e && v >= 1) return (size_t)std::min<unsigned long long>(v, kTrainMaxEpochsPerLaunch);
    }
    std::vector<double> per_group(grid, 0.0);
    for (size_t j = 0; j < items.size(); ++j) per_group[j % grid] += epoch_steps(items[j]);
    const double worst = *std::max_element(per_group.begin(), per_group.end());
    const double e = worst > 0.0 ? std::floor(kTrainStepsPerLaunch / worst) : (double)kTrainMaxEpochsPerLaunch;
    return (size_t)std::min(std::max(e, 1.0), (double)kTrainMaxEpochsPerLaunch);
}

size_t align4(size_t n) { return (n + 3) & ~(size_t)3; }
}  // namespace

bool train_mlp_batch(Ctx *ctx, const std::vector<MlpTrainItem> &items, float learning_rate, size_t epochs, TrainLeft *left) {
    if (left) left->jobs.clear();
    const size_t W = items.size();
    ctx->train_longest_launch_ms = 0.0; ctx->train_launches = 0;
    if (W == 0) return true;
    if (W > 0x7fffffffULL) { set_last_error("too many models in one call"); return false; }
    bool any_test = false;
    for (size_t w = 0; w < W; ++w) {
        const MlpTrainItem &it = items[w];
        const std::string who = "model " + std::to_string(w) + ": ";
        if (it.n_layers < 1 || it.n_layers > kTrainMaxLayers) { set_last_error(who + "an MLP of 1 to 4 layers is required"); return false; }
        size_t widest = 1;
        for (int l = 0; l <= it.n_layers; ++l) {
            if (it.dims[l] < 1) { set_last_error(who + "layer widths must be >= 1"); return false; }
            widest = std::max(widest, (size_t)it.dims[l]);
        }
        if (it.B < 1) { set_last_error(who + "no rows to train on"); return false; }
        // the kernel indexes a layer's result elements with an int and steps past the last one by up to four workgroup widths
        if ((widest + 1) * std::max(std::max(it.B, it.Bt), widest / 4 + 1) > 0x7fff0000ULL) { set_last_error(who + "rows x layer width beyond the kernel's range"); return false; }
        if (!it.x || !it.labels || !it.params || (it.tlog && it.Bt && !it.xt)) { set_last_error(who + "null argument"); return false; }
        for (size_t b = 0; b < it.B; ++b)
            if (it.labels[b] < 0 || it.labels[b] >= it.dims[it.n_layers]) { set_last_error(who + "label out of range"); return false; }
        any_test = any_test || (it.tlog && it.Bt);
    }
    // the workspace, in floats: job table | per model x, xt, labels | per model the weights and biases | loss rows | test logits |
    // act, dz.  The upload is everything up to the end of the weights, the download the weights, loss rows and test logits.
    std::vector<TrainJob> jobs(W);
    size_t at = W * sizeof(TrainJob) / sizeof(float);
    auto take = [&](size_t n) { const size_t o = at; at += align4(n); return (long long)o; };
    for (size_t w = 0; w < W; ++w) {
        const MlpTrainItem &it = items[w];
        TrainJob &j = jobs[w];
        std::memset(&j, 0, sizeof(j));
        j.n_layers = it.n_layers; j.B = (int)it.B; j.Bt = it.tlog ? (int)it.Bt : 0;
        for (int l = 0; l <= it.n_layers; ++l) j.dims[l] = it.dims[l];
        j.x = take(it.B * (size_t)it.dims[0]);
        j.xt = take((size_t)j.Bt * (size_t)it.dims[0]);
        j.labels = take(it.B);
    }
    const size_t params_at = at;
    for (size_t w = 0; w < W; ++w)
        for (int l = 0; l < items[w].n_layers; ++l) {
            jobs[w].w[l] = take((size_t)items[w].dims[l] * (size_t)items[w].dims[l + 1]);
            jobs[w].b[l] = take((size_t)items[w].dims[l + 1]);
        }
    const size_t upload_floats = at;
    for (size_t w = 0; w < W; ++w) jobs[w].loss = take(items[w].B);
    for (size_t w = 0; w < W; ++w) jobs[w].tlog = take((size_t)jobs[w].Bt * (size_t)items[w].dims[items[w].n_layers]);
    const size_t download_end = at;
    for (size_t w = 0; w < W; ++w)
        for (int l = 0; l < items[w].n_layers; ++l) {
            jobs[w].act[l] = take(std::max(items[w].B, (size_t)jobs[w].Bt) * (size_t)items[w].dims[l + 1]);
            jobs[w].dz[l] = take(items[w].B * (size_t)items[w].dims[l + 1]);
        }
    std::vector<float> img(download_end, 0.f);   // the upload's image, then the download's target
    std::memcpy(img.data(), jobs.data(), W * sizeof(TrainJob));
    parallel_for(W, [&](size_t w) {
        const MlpTrainItem &it = items[w];
        const TrainJob &j = jobs[w];
        std::memcpy(img.data() + j.x, it.x, it.B * (size_t)it.dims[0] * sizeof(float));
        if (j.Bt) std::memcpy(img.data() + j.xt, it.xt, (size_t)j.Bt * (size_t)it.dims[0] * sizeof(float));
        std::memcpy(img.data() + j.labels, it.labels, it.B * sizeof(int32_t));
        const float *src = it.params;
        for (int l = 0; l < it.n_layers; ++l) {
            const size_t nw = (size_t)it.dims[l] * (size_t)it.dims[l + 1], nb = (size_t)it.dims[l + 1];
            std::memcpy(img.data() + j.w[l], src, nw * sizeof(float)); src += nw;
            std::memcpy(img.data() + j.b[l], src, nb * sizeof(float)); src += nb;
        }
    });
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return false;
    hipStream_t st = ctx->stream;
    if (!ctx->ws_train.reserve(at * sizeof(float))) return false;
    float *ws = ctx->ws_train.as<float>();
    if (!hip_ok(hipMemcpyAsync(ws, img.data(), upload_floats * sizeof(float), hipMemcpyHostToDevice, st), "hipMemcpyAsync")) return false;
    const unsigned grid = (unsigned)std::min<size_t>(W, (size_t)std::max(ctx->n_cu, 1));
    const size_t E = epochs_per_launch(items, grid);
    std::vector<std::pair<hipEvent_t, hipEvent_t>> stamps;
    bool ok = true;
    auto launch = [&](int n_epochs, int test_forward, const char *what) {
        hipEvent_t a = nullptr, b = nullptr;
        const bool stamp = ctx->timing && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess;
        if (stamp) (void)hipEventRecord(a, st);
        ctx->time_begin(kKernelMlp);
        ok = hip_ok(launch_train_batch(st, reinterpret_cast<const TrainJob *>(ws), W, grid, ws, learning_rate, n_epochs, test_forward), what);
        ctx->time_end();
        if (stamp) { (void)hipEventRecord(b, st); stamps.emplace_back(a, b); }
        else { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
        ++ctx->train_launches;
        return ok;
    };
    // the test forward rides on the last launch of epochs (a launch of its own for a call of no epochs)
    for (size_t done = 0; ok && done < epochs;) {
        const size_t n = std::min(E, epochs - done);
        done += n;
        launch((int)n, any_test && done == epochs ? 1 : 0, "train_batch_kernel");
    }
    if (ok && epochs == 0 && any_test) launch(0, 1, "train_batch_kernel (test forward)");
    if (ok) ok = hip_ok(hipMemcpyAsync(img.data() + params_at, ws + params_at, (download_end - params_at) * sizeof(float), hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
    if (ok) ok = hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize");
    else (void)hipStreamSynchronize(st);   // the error of the launch stays the call's
    for (auto &s : stamps) {
        float ms = 0.f;
        if (ok && hipEventElapsedTime(&ms, s.first, s.second) == hipSuccess) ctx->train_longest_launch_ms = std::max(ctx->train_longest_launch_ms, (double)ms);
        (void)hipEventDestroy(s.first); (void)hipEventDestroy(s.second);
    }
    if (!ok) return false;
    parallel_for(W, [&](size_t w) {
        const MlpTrainItem &it = items[w];
        const TrainJob &j = jobs[w];
        float *dst = it.params;
        for (int l = 0; l < it.n_layers; ++l) {
            const size_t nw = (size_t)it.dims[l] * (size_t)it.dims[l + 1], nb = (size_t)it.dims[l + 1];
            std::memcpy(dst, img.data() + j.w[l], nw * sizeof(float)); dst += nw;
            std::memcpy(dst, img.data() + j.b[l], nb * sizeof(float)); dst += nb;
        }
        if (it.loss_rows && epochs) std::memcpy(it.loss_rows, img.data() + j.loss, it.B * sizeof(float));
        if (j.Bt) std::memcpy(it.tlog, img.data() + j.tlog, (size_t)j.Bt * (size_t)it.dims[it.n_layers] * sizeof(float));
    });
    if (left) left->jobs = std::move(jobs);   // the parameters stay where the last launch left them
    return true;
}

bool train_wakeword_models(Ctx *ctx, const rp_train_options &opt, size_t W, const uint64_t *seeds, const size_t *train_counts,
                           const char *const *train_names, const uint8_t *const *train_wavs, const size_t *train_lens,
                           const size_t *test_counts, const char *const *test_names, const uint8_t *const *test_wavs, const size_t *test_lens,
                           const WakewordModelData *const *prev, std::vector<WakewordModelData> *out, float *final_loss, float *test_accuracy,
                           size_t first_index, TrainLeft *left) {
    out->clear();
    if (left) left->jobs.clear();
    ctx->train_feature_ms = 0.0;
    if (W == 0) { ctx->train_longest_launch_ms = 0.0; ctx->train_launches = 0; return true; }
    // prepare.  The features go through compute_wav_mfccs one sample after the other: it works on the context's stream and caches, and a
    // batched MFCC front for training samples is not part of this call.
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<Prepared> prep(W);
    size_t tr = 0, te = 0;
    for (size_t w = 0; w < W; ++w) {
        rp_train_options o = opt;
        o.seed = seeds ? seeds[w] : opt.seed + (uint64_t)w;
        bool ok = prepare_model(ctx, o, train_counts[w], train_names + tr, train_wavs + tr, train_lens + tr, test_counts[w], test_names + te,
                                test_wavs + te, test_lens + te, prev ? prev[w] : nullptr, &prep[w]);
        // what the single call's launches refuse: a layer whose input row does not fit mlp_layer_kernel's 64 KB of LDS
        for (int l = 0; ok && l < prep[w].n_layers(); ++l)
            if ((size_t)prep[w].dims[l] * sizeof(float) > 64 * 1024) ok = hip_ok(hipErrorInvalidValue, opt.epochs ? "training step" : "test forward");
        if (!ok) { set_last_error("model " + std::to_string(first_index + w) + ": " + last_error()); return false; }
        tr += train_counts[w]; te += test_counts[w];
    }
    ctx->train_feature_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    parallel_for(W, [&](size_t w) { prepare_rows(&prep[w]); });
    // the epochs
    std::vector<MlpTrainItem> items(W);
    for (size_t w = 0; w < W; ++w) {
        Prepared &p = prep[w];
        MlpTrainItem &it = items[w];
        it.n_layers = p.n_layers();
        for (int l = 0; l <= it.n_layers; ++l) it.dims[l] = p.dims[l];
        it.B = p.ytr.size(); it.Bt = p.yte.size();
        it.x = p.xtr.data(); it.xt = p.xte.data(); it.labels = p.ytr.data();
        it.params = p.params.data(); it.loss_rows = p.loss_rows.data(); it.tlog = p.tlog.data();
    }
    if (!train_mlp_batch(ctx, items, opt.learning_rate, opt.epochs, left)) return false;
    // finish
    out->resize(W);
    parallel_for(W, [&](size_t w) {
        finish_model(prep[w], opt.epochs, &(*out)[w], final_loss ? final_loss + w : nullptr, test_accuracy ? test_accuracy + w : nullptr);
        prep[w] = Prepared();
    });
    return true;
}

}  // namespace rp
