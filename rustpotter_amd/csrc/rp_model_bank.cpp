// rp_model_bank.cpp -- personal wakeword MODELS: a bank of W wakeword models resident on the device (rp_model_bank_*): model_from_data,
// ModelBank::create, the bank that changes (reserve, put, train into the bank) and the accessors.  The calls in which stream s runs ITS model
// are in rp_bank_calls.cpp.  The model counterpart of rp_bank.cpp.  DESIGN.md section 4.4.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "rp_capi.h"

using namespace rp;

namespace rp {

bool model_layers(const WakewordModelData &model, int *n_layers, std::vector<int> *dims, std::vector<const float *> *wp,
                  std::vector<const float *> *bp, int *none_index) {
    // init_model, src/wakewords/nn/wakeword_nn.rs:165-389: Tiny has ln1,ln2; the others ln1..ln3
    std::string mt = model.m_type;
    std::transform(mt.begin(), mt.end(), mt.begin(), ::tolower);
    *n_layers = mt == "tiny" ? 2 : (mt == "small" || mt == "medium" || mt == "large") ? 3 : 0;
    if (*n_layers == 0) { set_last_error("Unknown model type"); return false; }
    dims->clear(); wp->clear(); bp->clear();
    for (int l = 0; l < *n_layers; ++l) {
        auto wi = model.weights.find("ln" + std::to_string(l + 1) + ".weight");
        auto bi = model.weights.find("ln" + std::to_string(l + 1) + ".bias");
        if (wi == model.weights.end() || bi == model.weights.end() || wi->second.first.size() != 2) {
            set_last_error("Incorrect model layers");  // wakeword_nn.rs:252-256
            return false;
        }
        if (l == 0) dims->push_back((int)wi->second.first[1]);
        else if ((int)wi->second.first[1] != dims->back()) { set_last_error("Incorrect model layers"); return false; }
        dims->push_back((int)wi->second.first[0]);
        if (bi->second.second.size() != wi->second.first[0]) { set_last_error("Incorrect model layers"); return false; }
        // the tensor must hold exactly out x in values (the dims are attacker-controlled: Model::create copies out*in floats)
        if (wi->second.first[0] == 0 || wi->second.first[1] == 0 || wi->second.first[0] > 0x7fffffffULL || wi->second.first[1] > 0x7fffffffULL ||
            wi->second.second.size() / wi->second.first[0] != wi->second.first[1] ||
            wi->second.second.size() % wi->second.first[0] != 0) { set_last_error("Incorrect model layers"); return false; }
        wp->push_back(wi->second.second.data());
        bp->push_back(bi->second.second.data());
    }
    *none_index = -1;
    for (size_t i = 0; i < model.labels.size(); ++i) if (model.labels[i] == "none") { *none_index = (int)i; break; }  // src/constants.rs:12
    return true;
}

Model *model_from_data(Ctx *ctx, const WakewordModelData &model, int *n_layers, std::vector<int> *dims, int *none_index) {
    std::vector<const float *> wp, bp;
    int ni = -1;
    if (!model_layers(model, n_layers, dims, &wp, &bp, &ni)) return nullptr;
    std::unique_ptr<Model> net(Model::create(ctx, *n_layers, dims->data(), wp.data(), bp.data()));
    if (!net) return nullptr;
    if (dims->back() != (int)model.labels.size()) { set_last_error("Incorrect model layers"); return nullptr; }
    *none_index = ni;
    return net.release();
}

// The bank's limits are the shapes mlp_route sends to mlp_windows_kernel: mfcc_size 16, windows of at most 256 frames, layer 1 and the tail
// layers at most 32 wide, a packed tail of at most 6144 floats.  Every refusal names its limit.  (mlp_route itself keeps windows of ONE
// frame, which the bank accepts, with mlp_mfma_kernel: rp_mlp.hip.)
bool ModelBank::entry_of(const std::vector<int> &dims, int ni, int image_ok, ModelBankEntry *out, std::string *why) {
    const int nl = (int)dims.size() - 1;
    auto fail = [&](const std::string &w) { *why = w; return false; };
    if (dims[0] % 16 != 0) return fail("an input of " + std::to_string(dims[0]) + " features is no whole number of frames of mfcc_size 16");
    const int L = dims[0] / 16;
    if (L > 256) return fail("a window of " + std::to_string(L) + " frames; the model bank takes windows of at most 256 frames");
    if (dims[1] > 32)
        return fail("layer 1 is " + std::to_string(dims[1]) + " wide; the model bank takes layer 1 at most 32 wide (every Tiny model, Small models up to 197 frames; Medium and Large models are not served from a bank)");
    for (int l = 2; l <= nl; ++l)
        if (dims[l] > 32) return fail("layer " + std::to_string(l) + " is " + std::to_string(dims[l]) + " wide; the model bank takes tail layers at most 32 wide");
    // what Model::create makes of these widths
    MlpDev d;
    d.n_layers = nl;
    for (int l = 0; l <= nl; ++l) d.dims[l] = dims[l];
    d.nt = dims[1] <= 16 ? 1 : 2;
    d.kpad = (dims[0] + 127) / 128 * 128;
    for (int l = 1; l < nl; ++l) d.tail_floats += (dims[l] + 1) * dims[l + 1];
    if (d.tail_floats == 0) d.tail_floats = 1;
    if (d.tail_floats > 6144) return fail("a packed tail of " + std::to_string(d.tail_floats) + " floats; the model bank takes at most 6144");
    if (image_ok < 0) image_ok = L >= 1 && mlp_mfma_fits(d) ? 1 : 0;
    if (!image_ok) return fail("this model has no three-part layer-1 image (mlp_windows_kernel does not take it)");
    if (ni < -1 || ni >= dims[nl]) return fail("none_index out of range");
    ModelBankEntry &e = *out;
    e = ModelBankEntry{};
    e.L = L; e.n1p = 16 * d.nt;
    e.n_layers = nl; e.d1 = d.dims[1]; e.d2 = d.dims[2]; e.d3 = d.dims[3];
    e.tail_floats = d.tail_floats; e.n_labels = dims[nl]; e.none_index = ni; e.pad = 0;
    return true;
}

// the pool space of one entry: [frame][3 parts][2 k-halves][32 outputs] 16-byte pieces (MlpDev::wwin3, one 32-output tile); b1; wsum; tail
static void entry_space(const ModelBankEntry &e, size_t n[4]) {
    n[ModelBank::kImg] = (size_t)e.L * 192; n[ModelBank::kB1] = (size_t)e.n1p; n[ModelBank::kWsum] = (size_t)e.n1p * 16;
    n[ModelBank::kTail] = (size_t)((e.tail_floats + 3) & ~3);
}
static const size_t kPoolUnit[4] = {16, 4, 4, 4};   // bytes

ModelBank *ModelBank::create(Ctx *ctx, size_t W, Model *const *models, int mfcc_size, const int32_t *none_index, const float *levels) {
    if (W > 0x7fffffffULL) { set_last_error("model bank: too many models"); return nullptr; }
    if (W && mfcc_size != 16) {
        set_last_error("model bank: mfcc_size " + std::to_string(mfcc_size) + " is not built (mlp_windows_bank_kernel takes mfcc_size 16)");
        return nullptr;
    }
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return nullptr;
    std::unique_ptr<ModelBank> b(new ModelBank());
    b->ctx = ctx;
    b->e.resize(W);
    b->rms_levels.assign(W, NAN);   // no level until the .rpw files or rp_model_bank_set_rms_levels give one
    if (levels) std::copy(levels, levels + W, b->rms_levels.begin());
    std::vector<BankWakeword> ww(W);
    size_t at[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < W; ++i) {
        auto fail = [&](const std::string &why) { set_last_error("model " + std::to_string(i) + ": " + why); return nullptr; };
        if (!models[i]) return fail("null handle");
        const Model &m = *models[i];
        const MlpDev &d = m.dev;
        if (m.ctx != ctx) return fail("the model belongs to another context");
        std::string why;
        ModelBankEntry &e = b->e[i];
        if (!entry_of(m.dims, none_index ? none_index[i] : -1, m.mfma_ok && d.wwin3 && d.b1 && d.tail ? 1 : 0, &e, &why)) return fail(why);
        e.wimg = (long long)at[kImg]; e.b1 = (long long)at[kB1]; e.wsum = (long long)at[kWsum]; e.tail = (long long)at[kTail];
        size_t n[4];
        entry_space(e, n);
        for (int k = 0; k < 4; ++k) at[k] += n[k];
        b->dev.label_pitch = std::max(b->dev.label_pitch, e.n_labels);
        b->max_L = std::max(b->max_L, e.L);
        b->min_L = i == 0 ? e.L : std::min(b->min_L, e.L);
        // the scan's view (bank_lane): the window, an avg row, the gates already applied by nn_score_bank_kernel (>=, not >)
        ww[i] = BankWakeword{0, 0, e.L, 0, 0, -1.f, -1.f, 0};
    }
    b->dev.W = (int)W;
    b->scan.W = (int)W; b->scan.K = 16; b->scan.max_len = b->max_L; b->scan.min_len = b->min_L;
    if (W == 0) return b.release();
    if (!b->d_e.reserve(W * sizeof(ModelBankEntry)) || !b->d_ww.reserve(W * sizeof(BankWakeword)) || !b->d_wimg.reserve(at[kImg] * 16) ||
        !b->d_b1.reserve(at[kB1] * 4) || !b->d_wsum.reserve(at[kWsum] * 4) || !b->d_tail.reserve(at[kTail] * 4) ||
        !b->d_level.reserve(W * sizeof(float))) return nullptr;
    auto d2d = [&](void *dst, const void *src, size_t bytes) {
        return hip_ok(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream), "hipMemcpyAsync(D2D)");
    };
    for (size_t i = 0; i < W; ++i) {
        Model &m = *models[i];
        const ModelBankEntry &e = b->e[i];
        const float *ws = m.wsum_for(16);
        if (!ws) return nullptr;
        if (!d2d(b->d_wimg.as<unsigned char>() + (size_t)e.wimg * 16, m.dev.wwin3, (size_t)e.L * 192 * 16) ||
            !d2d(b->d_b1.as<float>() + e.b1, m.dev.b1, (size_t)e.n1p * 4) || !d2d(b->d_wsum.as<float>() + e.wsum, ws, (size_t)e.n1p * 16 * 4) ||
            !d2d(b->d_tail.as<float>() + e.tail, m.dev.tail, (size_t)e.tail_floats * 4)) return nullptr;
    }
    if (!hip_ok(hipMemcpyAsync(b->d_e.p, b->e.data(), W * sizeof(ModelBankEntry), hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync(H2D)") ||
        !hip_ok(hipMemcpyAsync(b->d_ww.p, ww.data(), W * sizeof(BankWakeword), hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync(H2D)") ||
        !hip_ok(hipMemcpyAsync(b->d_level.p, b->rms_levels.data(), W * sizeof(float), hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync(H2D)") ||
        !hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) return nullptr;   // the handles may be freed when this returns
    b->dev.e = b->d_e.as<ModelBankEntry>();
    b->dev.wimg = b->d_wimg.p;
    b->dev.b1 = b->d_b1.as<float>(); b->dev.wsum = b->d_wsum.as<float>(); b->dev.tail = b->d_tail.as<float>();
    b->scan.ww = b->d_ww.as<BankWakeword>();
    // the pools start exactly full (rp_host.h: a bank that grows)
    for (int k = 0; k < 4; ++k) b->used[k] = b->cap[k] = at[k];
    b->cap_models = W;
    return b.release();
}

bool ModelBank::set_rms_levels(const float *levels) {
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return false;
    if (rms_levels.empty()) return true;
    std::copy(levels, levels + rms_levels.size(), rms_levels.begin());
    // behind whatever the context's stream still runs with the old levels; the host copy is the bank's own, so it may change again at once
    return hip_ok(hipMemcpyAsync(d_level.p, rms_levels.data(), rms_levels.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream),
                  "hipMemcpyAsync(rms levels)") && hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
}

// ---------------------------------------------------------------------------------------------------------------- a bank that grows
bool ModelBank::put_check(size_t first, const std::vector<PutItem> &items, const char *who) const {
    if (first > (size_t)dev.W) {
        set_last_error("first model index " + std::to_string(first) + " is past the bank's " + std::to_string(dev.W) + " models: a bank has no holes");
        return false;
    }
    if (items.size() > 0x7fffffffULL - first) { set_last_error("model bank: too many models"); return false; }
    const int largest = dev.label_pitch;   // without a reservation: the largest label count (under a batch: the largest there has been)
    for (size_t i = 0; i < items.size(); ++i) {
        const ModelBankEntry &x = items[i].entry;
        auto fail = [&](const std::string &why) { set_last_error(std::string(who) + " " + std::to_string(first + i) + ": " + why); return false; };
        // a stream batch sized its MFCC history and its logits once: the bank never comes to hold a model it has no room for
        if (res_L && x.L > res_L)
            return fail("a window of " + std::to_string(x.L) + " frames is longer than the bank's reserved train size (" + std::to_string(res_L) + " frames, rp_model_bank_reserve)");
        if (res_labels && x.n_labels > res_labels)
            return fail(std::to_string(x.n_labels) + " labels are more than the bank's reserved label count (" + std::to_string(res_labels) + ", rp_model_bank_reserve)");
        if (!res_L && live_batches && x.L > max_L)
            return fail("a window of " + std::to_string(x.L) + " frames is longer than the bank's longest (" + std::to_string(max_L) +
                        " frames) while a stream batch runs over the bank: call rp_model_bank_reserve before creating the batch");
        if (!res_labels && live_batches && x.n_labels > largest)
            return fail(std::to_string(x.n_labels) + " labels are more than the bank's largest label count (" + std::to_string(largest) +
                        ") while a stream batch runs over the bank: call rp_model_bank_reserve before creating the batch");
    }
    return true;
}

// swaps a pool for its replacement; the old memory goes when `fresh` does
static void take_over(DevBuf &pool, DevBuf &fresh) { std::swap(pool.p, fresh.p); std::swap(pool.cap, fresh.cap); }

bool ModelBank::grow_models(size_t n) {
    if (n <= cap_models) return true;
    DevBuf ne, nw, nl;   // the levels move with the descriptors
    const size_t W = (size_t)dev.W;
    // behind whatever still reads the old arrays; they are freed after the stream has drained
    if (!ne.reserve(n * sizeof(ModelBankEntry)) || !nw.reserve(n * sizeof(BankWakeword)) || !nl.reserve(n * sizeof(float)) ||
        (W && (!hip_ok(hipMemcpyAsync(nl.p, d_level.p, W * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream), "hipMemcpyAsync(model bank)") ||
               !hip_ok(hipMemcpyAsync(ne.p, d_e.p, W * sizeof(ModelBankEntry), hipMemcpyDeviceToDevice, ctx->stream), "hipMemcpyAsync(model bank)") ||
               !hip_ok(hipMemcpyAsync(nw.p, d_ww.p, W * sizeof(BankWakeword), hipMemcpyDeviceToDevice, ctx->stream), "hipMemcpyAsync(model bank)"))) ||
        !hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) return false;
    take_over(d_e, ne); take_over(d_ww, nw); take_over(d_level, nl);
    dev.e = d_e.as<ModelBankEntry>(); scan.ww = d_ww.as<BankWakeword>();
    cap_models = n;
    return true;
}

// Growth is the compaction: the live models, in index order, get consecutive places in the new pools; what replaced models left behind stays
// in the old ones.
bool ModelBank::repool(const size_t want[4]) {
    std::vector<ModelBankEntry> ne(e);
    size_t at[4] = {0, 0, 0, 0};
    for (ModelBankEntry &x : ne) {
        size_t n[4];
        entry_space(x, n);
        x.wimg = (long long)at[kImg]; x.b1 = (long long)at[kB1]; x.wsum = (long long)at[kWsum]; x.tail = (long long)at[kTail];
        for (int k = 0; k < 4; ++k) at[k] += n[k];
    }
    for (int k = 0; k < 4; ++k)
        if (at[k] > want[k]) { set_last_error("model bank: pool too small for its live models"); return false; }
    DevBuf fresh[4];
    for (int k = 0; k < 4; ++k)
        if (!fresh[k].reserve(std::max<size_t>(want[k], 1) * kPoolUnit[k])) return false;
    const size_t W = ne.size();
    const hipStream_t st = ctx->stream;
    if (W) {
        // the relocation table: from | to
        if (!put_ws.reserve(2 * W * sizeof(ModelBankEntry))) return false;
        ModelBankEntry *t_from = put_ws.as<ModelBankEntry>(), *t_to = t_from + W;
        ModelBankMove m;
        m.from = t_from; m.to = t_to; m.n = W;
        m.wimg_old = d_wimg.p; m.b1_old = d_b1.as<float>(); m.wsum_old = d_wsum.as<float>(); m.tail_old = d_tail.as<float>();
        m.wimg_new = fresh[kImg].p; m.b1_new = fresh[kB1].as<float>(); m.wsum_new = fresh[kWsum].as<float>(); m.tail_new = fresh[kTail].as<float>();
        if (!hip_ok(hipMemcpyAsync(t_from, e.data(), W * sizeof(ModelBankEntry), hipMemcpyHostToDevice, st), "hipMemcpyAsync(model bank)") ||
            !hip_ok(hipMemcpyAsync(t_to, ne.data(), W * sizeof(ModelBankEntry), hipMemcpyHostToDevice, st), "hipMemcpyAsync(model bank)") ||
            !hip_ok(launch_model_bank_move(st, m), "model_bank_move_kernel") ||
            !hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize")) { (void)hipStreamSynchronize(st); return false; }
        // nothing in flight reads the bank any more: the descriptors and the pools change together
        if (!hip_ok(hipMemcpy(d_e.p, ne.data(), W * sizeof(ModelBankEntry), hipMemcpyHostToDevice), "hipMemcpy(model bank)")) {
            (void)hipMemcpy(d_e.p, e.data(), W * sizeof(ModelBankEntry), hipMemcpyHostToDevice);
            return false;
        }
    } else if (!hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize")) return false;
    take_over(d_wimg, fresh[kImg]); take_over(d_b1, fresh[kB1]); take_over(d_wsum, fresh[kWsum]); take_over(d_tail, fresh[kTail]);
    dev.wimg = d_wimg.p; dev.b1 = d_b1.as<float>(); dev.wsum = d_wsum.as<float>(); dev.tail = d_tail.as<float>();
    e.swap(ne);
    for (int k = 0; k < 4; ++k) { used[k] = at[k]; dead[k] = 0; cap[k] = want[k]; }
    ++grown;
    return true;
}

bool ModelBank::reserve(int max_train_size, int max_labels, size_t n_models, size_t n_frames) {
    if (max_train_size < 0 || max_labels < 0) { set_last_error("rp_model_bank_reserve: max_train_size and max_labels must be >= 0"); return false; }
    int largest = 0;
    for (const ModelBankEntry &x : e) largest = std::max(largest, x.n_labels);
    if ((max_train_size && max_train_size != res_L) || (max_labels && max_labels != res_labels)) {
        if (live_batches) { set_last_error("rp_model_bank_reserve: the reserved train size and label count can only change while no stream batch runs over the bank"); return false; }
        if (max_train_size && max_train_size < max_L) {
            set_last_error("rp_model_bank_reserve: max_train_size " + std::to_string(max_train_size) + " is below the bank's longest window (" + std::to_string(max_L) + " frames)");
            return false;
        }
        if (max_train_size > 256) { set_last_error("rp_model_bank_reserve: max_train_size " + std::to_string(max_train_size) + "; the model bank takes windows of at most 256 frames"); return false; }
        if (max_labels && max_labels < largest) {
            set_last_error("rp_model_bank_reserve: max_labels " + std::to_string(max_labels) + " is below the bank's largest label count (" + std::to_string(largest) + ")");
            return false;
        }
        if (max_labels > 32) { set_last_error("rp_model_bank_reserve: max_labels " + std::to_string(max_labels) + "; the model bank takes tail layers at most 32 wide"); return false; }
    }
    if (n_models > 0x7fffffffULL || n_frames > (size_t)1 << 40) { set_last_error("model bank: too many models"); return false; }
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return false;
    // hints, never limits: 32 rows of b1 and wsum a model at the most; 1024 floats of tail hold every Tiny model and the usual Small one
    const size_t want[4] = {std::max(cap[kImg], n_frames * 192), std::max(cap[kB1], n_models * 32), std::max(cap[kWsum], n_models * 512),
                            std::max(cap[kTail], n_models * 1024)};
    if (!grow_models(n_models)) return false;
    bool more = false;
    for (int k = 0; k < 4; ++k) more = more || want[k] > cap[k];
    if (more && !repool(want)) return false;
    if (max_train_size) res_L = max_train_size;
    if (max_labels) res_labels = max_labels;
    dev.label_pitch = std::max(res_labels, largest);
    return true;
}

bool ModelBank::put(size_t first, const std::vector<PutItem> &items, const char *who) {
    const size_t n = items.size();
    last_put_ms = 0.0;
    if (n == 0) return true;
    size_t need[4] = {0, 0, 0, 0};
    int call_L = 1, call_tail = 0;
    for (const PutItem &it : items) {
        size_t sp[4];
        entry_space(it.entry, sp);
        for (int k = 0; k < 4; ++k) need[k] += sp[k];
        call_L = std::max(call_L, it.entry.L); call_tail = std::max(call_tail, (int)sp[kTail]);
    }
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return false;
    // room: a pool that is full is replaced by one at least twice its size (which drops the garbage)
    if (!grow_models(first + n > cap_models ? std::max(first + n, 2 * cap_models) : cap_models)) return false;
    bool is_short = false;
    size_t want[4];
    for (int k = 0; k < 4; ++k) {
        const bool s = used[k] + need[k] > cap[k];
        want[k] = s ? std::max(2 * cap[k], used[k] - dead[k] + need[k]) : cap[k];
        is_short = is_short || s;
    }
    if (is_short && !repool(want)) return false;
    // the new entries, model after model, in the pool tails: nothing in flight reads them
    std::vector<ModelPutItem> tab(n);
    std::vector<ModelBankEntry> ne(n);
    std::vector<BankWakeword> nww(n);
    std::vector<float> nlevel(n);
    size_t at[4] = {used[0], used[1], used[2], used[3]};
    for (size_t i = 0; i < n; ++i) {
        ModelBankEntry &x = ne[i];
        x = items[i].entry;
        x.wimg = (long long)at[kImg]; x.b1 = (long long)at[kB1]; x.wsum = (long long)at[kWsum]; x.tail = (long long)at[kTail];
        size_t sp[4];
        entry_space(x, sp);
        for (int k = 0; k < 4; ++k) at[k] += sp[k];
        for (int l = 0; l < 3; ++l) { tab[i].w[l] = items[i].w[l]; tab[i].b[l] = items[i].b[l]; }
        tab[i].e = x;
        nww[i] = BankWakeword{0, 0, x.L, 0, 0, -1.f, -1.f, 0};
        nlevel[i] = items[i].rms_level;
    }
    const size_t tab_bytes = n * sizeof(ModelPutItem);
    if (!put_ws.reserve(tab_bytes + n * sizeof(uint32_t))) return false;
    ModelBankPut p;
    p.items = put_ws.as<ModelPutItem>(); p.n = n; p.max_L = call_L; p.max_tail = call_tail;
    p.wimg = d_wimg.p; p.b1 = d_b1.as<float>(); p.wsum = d_wsum.as<float>(); p.tail = d_tail.as<float>();
    p.flags = reinterpret_cast<uint32_t *>(put_ws.as<char>() + tab_bytes);
    std::vector<uint32_t> flags(n);
    const hipStream_t st = ctx->stream;
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    const bool stamp = ctx->timing && hipEventCreate(&ev_a) == hipSuccess && hipEventCreate(&ev_b) == hipSuccess;
    auto drop_events = [&] { if (ev_a) (void)hipEventDestroy(ev_a); if (ev_b) (void)hipEventDestroy(ev_b); };
    bool ok = hip_ok(hipMemcpyAsync(put_ws.p, tab.data(), tab_bytes, hipMemcpyHostToDevice, st), "hipMemcpyAsync(model bank)") &&
              hip_ok(hipMemsetAsync(p.flags, 0, n * sizeof(uint32_t), st), "hipMemsetAsync");
    if (ok && stamp) (void)hipEventRecord(ev_a, st);
    ok = ok && hip_ok(launch_model_bank_put(st, p), "model_bank_put_kernel");
    if (ok && stamp) (void)hipEventRecord(ev_b, st);
    ok = ok && hip_ok(hipMemcpyAsync(flags.data(), p.flags, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync(model bank)");
    if (ok) ok = hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize");
    else (void)hipStreamSynchronize(st);
    if (ok && stamp) { float ms = 0.f; if (hipEventElapsedTime(&ms, ev_a, ev_b) == hipSuccess) last_put_ms = ms; }
    drop_events();
    if (!ok) return false;
    for (size_t i = 0; i < n; ++i)
        if (flags[i] & kModelPutNotFinite) { set_last_error(std::string(who) + " " + std::to_string(first + i) + ": parameters must be finite"); return false; }
    // commit: the descriptors -- behind every launch that took the bank as it was
    if (!hip_ok(hipMemcpyAsync(d_e.as<ModelBankEntry>() + first, ne.data(), n * sizeof(ModelBankEntry), hipMemcpyHostToDevice, st), "hipMemcpyAsync(model bank)") ||
        !hip_ok(hipMemcpyAsync(d_ww.as<BankWakeword>() + first, nww.data(), n * sizeof(BankWakeword), hipMemcpyHostToDevice, st), "hipMemcpyAsync(model bank)") ||
        !hip_ok(hipMemcpyAsync(d_level.as<float>() + first, nlevel.data(), n * sizeof(float), hipMemcpyHostToDevice, st), "hipMemcpyAsync(model bank)") ||
        !hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize")) return false;
    for (size_t w = first; w < std::min(first + n, e.size()); ++w) {   // what a replaced model leaves behind
        size_t sp[4];
        entry_space(e[w], sp);
        for (int k = 0; k < 4; ++k) dead[k] += sp[k];
    }
    for (int k = 0; k < 4; ++k) used[k] = at[k];
    if (e.size() < first + n) { e.resize(first + n); rms_levels.resize(first + n, NAN); }
    std::copy(ne.begin(), ne.end(), e.begin() + (long)first);
    std::copy(nlevel.begin(), nlevel.end(), rms_levels.begin() + (long)first);
    dev.W = (int)e.size();
    int largest = 0;
    max_L = min_L = 0;
    for (size_t w = 0; w < e.size(); ++w) {
        max_L = std::max(max_L, e[w].L);
        min_L = w == 0 ? e[w].L : std::min(min_L, e[w].L);
        largest = std::max(largest, e[w].n_labels);
    }
    // the pitch of a live batch's logits never changes under it: a replaced model may leave it larger than the bank needs
    dev.label_pitch = live_batches ? std::max(dev.label_pitch, std::max(res_labels, largest)) : std::max(res_labels, largest);
    scan.W = dev.W; scan.K = 16; scan.max_len = max_L; scan.min_len = min_L;
    return true;
}

}  // namespace rp

namespace {

int bank_handle(std::unique_ptr<ModelBank> b, rp_model_bank **out) {
    if (!b) return -1;
    rp_model_bank *h = new rp_model_bank();
    h->impl = std::move(b);
    *out = h;
    return 0;
}

const char kNotBuilt[] = " is not built (mlp_windows_bank_kernel takes mfcc_size 16)";

// the raw parameters of the call's models on the host, every tensor at a multiple of 4 floats (16 bytes) of one block
struct RawParams {
    std::vector<float> block;
    std::vector<size_t> w_at, b_at;   // [model][3]
    size_t add(const float *src, size_t n) {
        const size_t at = block.size();
        block.resize(at + ((n + 3) & ~(size_t)3), 0.f);
        std::memcpy(block.data() + at, src, n * sizeof(float));
        return at;
    }
};

// what a model of these widths is to the bank, or the refusal behind "<who> <index>: "
bool put_item_of(const std::vector<int> &dims, int none_index, int image_ok, const char *who, size_t index, ModelBank::PutItem *it) {
    std::string why;
    if (ModelBank::entry_of(dims, none_index, image_ok, &it->entry, &why)) return true;
    set_last_error(std::string(who) + " " + std::to_string(index) + ": " + why);
    return false;
}

}  // namespace

extern "C" {

int rp_model_bank_new(rp_ctx *ctx, size_t n_models, const rp_model *const *models, int mfcc_size, const int32_t *none_index, rp_model_bank **out) {
    return guarded([&]() -> int {
        if (!ctx || !out) { set_last_error("null argument"); return -1; }
        *out = nullptr;
        if (n_models && !models) { set_last_error("null argument"); return -1; }
        std::vector<Model *> ms(n_models, nullptr);
        for (size_t i = 0; i < n_models; ++i) ms[i] = models[i] ? models[i]->impl.get() : nullptr;
        return bank_handle(std::unique_ptr<ModelBank>(ModelBank::create(ctx->impl.get(), n_models, ms.data(), mfcc_size, none_index)), out);
    });
}

int rp_model_bank_new_from_rpw(rp_ctx *ctx, size_t n_models, const uint8_t *const *rpw_buffers, const size_t *rpw_lens, rp_model_bank **out) {
    return guarded([&]() -> int {
        if (!ctx || !out) { set_last_error("null argument"); return -1; }
        *out = nullptr;
        if (n_models && (!rpw_buffers || !rpw_lens)) { set_last_error("null argument"); return -1; }
        Ctx *c = ctx->impl.get();
        std::vector<std::unique_ptr<Model>> owned;
        std::vector<Model *> ms;
        std::vector<int32_t> none;
        std::vector<float> levels;
        int K = 0;
        for (size_t w = 0; w < n_models; ++w) {
            auto fail = [&](const std::string &why) { set_last_error("wakeword " + std::to_string(w) + ": " + why); return -1; };
            if (!rpw_buffers[w]) return fail("null buffer");
            RpwKind kind;
            WakewordRefData ref;
            WakewordModelData model;
            std::string err;
            if (!parse_rpw(rpw_buffers[w], rpw_lens[w], &kind, &ref, &model, &err)) return fail(err);
            if (kind != RpwKind::Model) return fail("a wakeword reference cannot be part of a model bank (wakeword models only)");
            if (K == 0) K = model.mfcc_size;
            else if (model.mfcc_size != K) return fail("Usage of wakewords with different mfcc size is not supported, ignoring wakeword");
            int n_layers = 0, ni = -1;
            std::vector<int> dims;
            std::unique_ptr<Model> m(model_from_data(c, model, &n_layers, &dims, &ni));
            if (!m) return fail(last_error());
            ms.push_back(m.get());
            owned.push_back(std::move(m));
            none.push_back(ni);
            levels.push_back(model.rms_level);
        }
        return bank_handle(std::unique_ptr<ModelBank>(ModelBank::create(c, n_models, ms.data(), n_models ? K : 16, none.data(), levels.data())), out);
    });
}

void rp_model_bank_free(rp_model_bank *bank) { delete bank; }

int rp_model_bank_size(const rp_model_bank *bank) { return bank ? bank->impl->dev.W : -1; }

int rp_model_bank_train_size(const rp_model_bank *bank, long long model) {
    if (!bank || model >= (long long)bank->impl->dev.W) return -1;
    return model < 0 ? bank->impl->max_L : bank->impl->e[(size_t)model].L;
}

int rp_model_bank_labels(const rp_model_bank *bank, long long model) {
    if (!bank || model >= (long long)bank->impl->dev.W) return -1;
    return model < 0 ? bank->impl->dev.label_pitch : bank->impl->e[(size_t)model].n_labels;
}

int rp_model_bank_reserve(rp_model_bank *bank, int max_train_size, int max_labels, size_t n_models, size_t n_frames) {
    return guarded([&]() -> int {
        if (!bank) { set_last_error("null handle"); return -1; }
        return bank->impl->reserve(max_train_size, max_labels, n_models, n_frames) ? 0 : -1;
    });
}

int rp_model_bank_reserved(const rp_model_bank *bank, int *max_train_size, int *max_labels) {
    if (!bank) { set_last_error("null handle"); return -1; }
    if (max_train_size) *max_train_size = bank->impl->res_L;
    if (max_labels) *max_labels = bank->impl->res_labels;
    return 0;
}

int rp_model_bank_pool_growths(const rp_model_bank *bank) {
    if (!bank) { set_last_error("null handle"); return -1; }
    return (int)std::min<size_t>(bank->impl->grown, 0x7fffffff);
}

int rp_model_bank_set_rms_levels(rp_model_bank *bank, const float *rms_levels) {
    return guarded([&]() -> int {
        if (!bank) { set_last_error("null handle"); return -1; }
        if (!rms_levels && bank->impl->dev.W) { set_last_error("null argument"); return -1; }
        return bank->impl->set_rms_levels(rms_levels) ? 0 : -1;
    });
}

float rp_model_bank_rms_level(const rp_model_bank *bank, long long model) {
    if (!bank || model < 0 || model >= (long long)bank->impl->dev.W) return NAN;
    return bank->impl->rms_levels[(size_t)model];
}

double rp_model_bank_last_put_ms(const rp_model_bank *bank) { return bank ? bank->impl->last_put_ms : 0.0; }

int rp_model_bank_put(rp_model_bank *bank, size_t first, size_t n, const rp_model *const *models, const int32_t *none_index) {
    return guarded([&]() -> int {
        if (!bank) { set_last_error("null handle"); return -1; }
        if (n == 0) return 0;
        if (!models) { set_last_error("null argument"); return -1; }
        ModelBank &bk = *bank->impl;
        if (!bk.put_check(first, {}, "model")) return -1;
        std::vector<ModelBank::PutItem> items(n);
        for (size_t i = 0; i < n; ++i) {
            auto fail = [&](const std::string &why) { set_last_error("model " + std::to_string(first + i) + ": " + why); return -1; };
            if (!models[i]) return fail("null handle");
            const Model &m = *models[i]->impl;
            if (m.ctx != bk.ctx) return fail("the model belongs to another context");
            if (m.dims.size() < 2 || m.dims.size() > 4) return fail("Incorrect model layers");
            if (!put_item_of(m.dims, none_index ? none_index[i] : -1, m.mfma_ok && m.dev.wwin3 && m.dev.b1 && m.dev.tail ? 1 : 0, "model", first + i, &items[i])) return -1;
            for (size_t l = 0; l + 1 < m.dims.size(); ++l) { items[i].w[l] = m.W[l]; items[i].b[l] = m.B[l]; }
        }
        if (!bk.put_check(first, items, "model")) return -1;
        return bk.put(first, items, "model") ? 0 : -1;
    });
}

int rp_model_bank_put_from_rpw(rp_model_bank *bank, size_t first, size_t n, const uint8_t *const *rpw_buffers, const size_t *rpw_lens) {
    return guarded([&]() -> int {
        if (!bank) { set_last_error("null handle"); return -1; }
        if (n == 0) return 0;
        if (!rpw_buffers || !rpw_lens) { set_last_error("null argument"); return -1; }
        ModelBank &bk = *bank->impl;
        Ctx *c = bk.ctx;
        if (!bk.put_check(first, {}, "wakeword")) return -1;
        std::vector<ModelBank::PutItem> items(n);
        RawParams raw;
        int K = 0;
        for (size_t w = 0; w < n; ++w) {
            auto fail = [&](const std::string &why) { set_last_error("wakeword " + std::to_string(first + w) + ": " + why); return -1; };
            if (!rpw_buffers[w]) return fail("null buffer");
            RpwKind kind;
            WakewordRefData ref;
            WakewordModelData model;
            std::string err;
            if (!parse_rpw(rpw_buffers[w], rpw_lens[w], &kind, &ref, &model, &err)) return fail(err);
            if (kind != RpwKind::Model) return fail("a wakeword reference cannot be part of a model bank (wakeword models only)");
            if (K == 0) K = model.mfcc_size;
            else if (model.mfcc_size != K) return fail("Usage of wakewords with different mfcc size is not supported, ignoring wakeword");
            int n_layers = 0, ni = -1;
            std::vector<int> dims;
            std::vector<const float *> wp, bp;
            if (!model_layers(model, &n_layers, &dims, &wp, &bp, &ni)) return fail(last_error());
            if (dims.back() != (int)model.labels.size()) return fail("Incorrect model layers");
            if (K != 16) { set_last_error("model bank: mfcc_size " + std::to_string(K) + kNotBuilt); return -1; }
            if (!put_item_of(dims, ni, -1, "wakeword", first + w, &items[w])) return -1;
            items[w].rms_level = model.rms_level;
            for (int l = 0; l < n_layers; ++l) {
                raw.w_at.push_back(raw.add(wp[l], (size_t)dims[l] * (size_t)dims[l + 1]));
                raw.b_at.push_back(raw.add(bp[l], (size_t)dims[l + 1]));
            }
            for (int l = n_layers; l < 3; ++l) { raw.w_at.push_back(0); raw.b_at.push_back(0); }
        }
        if (!bk.put_check(first, items, "wakeword")) return -1;
        // one upload of every model's parameters; model_bank_put_kernel reads them where they land
        if (!hip_ok(hipSetDevice(c->device), "hipSetDevice") || !c->stage_in.reserve(raw.block.size() * sizeof(float))) return -1;
        const float *d = c->stage_in.as<float>();
        if (!hip_ok(hipMemcpyAsync(c->stage_in.p, raw.block.data(), raw.block.size() * sizeof(float), hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync(H2D)")) return -1;
        for (size_t w = 0; w < n; ++w)
            for (int l = 0; l < items[w].entry.n_layers; ++l) { items[w].w[l] = d + raw.w_at[3 * w + l]; items[w].b[l] = d + raw.b_at[3 * w + l]; }
        const bool ok = bk.put(first, items, "wakeword");
        if (!ok) (void)hipStreamSynchronize(c->stream);   // the upload reads `raw`
        return ok ? 0 : -1;
    });
}

int rp_model_bank_train(rp_model_bank *bank, size_t first, size_t n, const rp_train_options *options, const uint64_t *seeds,
                        const size_t *train_counts, const char *const *train_names, const uint8_t *const *train_wavs, const size_t *train_lens,
                        const size_t *test_counts, const char *const *test_names, const uint8_t *const *test_wavs, const size_t *test_lens,
                        const uint8_t *const *prev_models, const size_t *prev_model_lens, uint8_t **out_rpw, size_t *out_lens, float *final_loss,
                        float *test_accuracy) {
    return guarded([&]() -> int {
        if (!bank) { set_last_error("null handle"); return -1; }
        if ((out_rpw != nullptr) != (out_lens != nullptr)) { set_last_error("null argument"); return -1; }
        if (n && (!options || !train_counts || !test_counts || (prev_models && !prev_model_lens))) { set_last_error("null argument"); return -1; }
        size_t n_train = 0, n_test = 0;
        for (size_t w = 0; w < n; ++w) { if (out_rpw) { out_rpw[w] = nullptr; out_lens[w] = 0; } n_train += train_counts[w]; n_test += test_counts[w]; }
        if ((n_train && (!train_names || !train_wavs || !train_lens)) || (n_test && (!test_names || !test_wavs || !test_lens))) {
            set_last_error("null argument");
            return -1;
        }
        if (n == 0) return 0;
        ModelBank &bk = *bank->impl;
        Ctx *c = bk.ctx;
        if (!bk.put_check(first, {}, "model")) return -1;   // `first` alone, before the work of a training
        if (options->mfcc_size != 16) { set_last_error("model bank: mfcc_size " + std::to_string(options->mfcc_size) + kNotBuilt); return -1; }
        std::vector<WakewordModelData> prev(prev_models ? n : 0), models;
        std::vector<const WakewordModelData *> prev_of(n, nullptr);
        for (size_t w = 0; prev_models && w < n; ++w) {
            if (!prev_models[w]) continue;
            const std::string who = "model " + std::to_string(first + w) + ": ";
            RpwKind kind; WakewordRefData ref; std::string err;
            if (!parse_rpw(prev_models[w], prev_model_lens[w], &kind, &ref, &prev[w], &err)) { set_last_error(who + err); return -1; }
            if (kind != RpwKind::Model) { set_last_error(who + "the file to train from is not a wakeword model"); return -1; }
            if (prev[w].mfcc_size != 16) { set_last_error(who + "model bank: mfcc_size " + std::to_string(prev[w].mfcc_size) + kNotBuilt); return -1; }
            prev_of[w] = &prev[w];
        }
        // rp_wakeword_model_train_batch's stages; the trained parameters stay in the training workspace
        TrainLeft left;
        if (!train_wakeword_models(c, *options, n, seeds, train_counts, train_names, train_wavs, train_lens, test_counts, test_names, test_wavs,
                                   test_lens, prev_of.data(), &models, final_loss, test_accuracy, first, &left)) return -1;
        std::vector<ModelBank::PutItem> items(n);
        const float *ws = c->ws_train.as<float>();
        for (size_t w = 0; w < n; ++w) {
            int n_layers = 0, ni = -1;
            std::vector<int> dims;
            std::vector<const float *> wp, bp;
            if (!model_layers(models[w], &n_layers, &dims, &wp, &bp, &ni)) { set_last_error("model " + std::to_string(first + w) + ": " + last_error()); return -1; }
            if (!put_item_of(dims, ni, -1, "model", first + w, &items[w])) return -1;
            items[w].rms_level = models[w].rms_level;   // the level the trained file carries (rp_train.cpp)
            for (int l = 0; l < n_layers; ++l) { items[w].w[l] = ws + left.jobs[w].w[l]; items[w].b[l] = ws + left.jobs[w].b[l]; }
        }
        if (!bk.put_check(first, items, "model")) return -1;
        // the files, when asked for: exactly rp_wakeword_model_train_batch's bytes, finished before the bank changes
        std::vector<std::vector<uint8_t>> bytes(out_rpw ? n : 0);
        if (out_rpw) parallel_for(n, [&](size_t w) { bytes[w] = serialize_wakeword_model(models[w]); });
        auto drop = [&] { for (size_t w = 0; out_rpw && w < n; ++w) { std::free(out_rpw[w]); out_rpw[w] = nullptr; out_lens[w] = 0; } return -1; };
        for (size_t w = 0; out_rpw && w < n; ++w) {
            out_rpw[w] = static_cast<uint8_t *>(std::malloc(std::max<size_t>(bytes[w].size(), 1)));
            if (!out_rpw[w]) { set_last_error("out of host memory"); return drop(); }
            std::memcpy(out_rpw[w], bytes[w].data(), bytes[w].size());
            out_lens[w] = bytes[w].size();
        }
        // from the workspace into the bank, on the stream the training ran on, before anything reuses the workspace
        if (!bk.put(first, items, "model")) return drop();
        return 0;
    });
}

int rp_model_bank_read_image(const rp_model_bank *bank, long long model, void *out, size_t cap, size_t *need) {
    return guarded([&]() -> int {
        if (!bank) { set_last_error("null handle"); return -1; }
        const ModelBank &bk = *bank->impl;
        if (model < 0 || model >= (long long)bk.dev.W) { set_last_error("model index outside the bank"); return -1; }
        const ModelBankEntry &e = bk.e[(size_t)model];
        const size_t n_img = (size_t)e.L * 192 * 16, n_b1 = (size_t)e.n1p * 4, n_sum = (size_t)e.n1p * 64, n_tail = (size_t)e.tail_floats * 4,
                     pitch = (size_t)((e.tail_floats + 3) & ~3) * 4, total = n_img + n_b1 + n_sum + pitch;
        if (need) *need = total;
        if (!out) return 0;
        if (cap < total) { set_last_error("rp_model_bank_read_image: the buffer is smaller than the image (" + std::to_string(total) + " bytes)"); return -1; }
        if (!hip_ok(hipSetDevice(bk.ctx->device), "hipSetDevice")) return -1;
        unsigned char *o = static_cast<unsigned char *>(out);
        const hipStream_t st = bk.ctx->stream;
        std::memset(o + n_img + n_b1 + n_sum + n_tail, 0, pitch - n_tail);   // behind the tail the pool holds nothing anybody reads
        if (!hip_ok(hipMemcpyAsync(o, bk.d_wimg.as<unsigned char>() + (size_t)e.wimg * 16, n_img, hipMemcpyDeviceToHost, st), "hipMemcpyAsync(D2H)") ||
            !hip_ok(hipMemcpyAsync(o + n_img, bk.d_b1.as<float>() + e.b1, n_b1, hipMemcpyDeviceToHost, st), "hipMemcpyAsync(D2H)") ||
            !hip_ok(hipMemcpyAsync(o + n_img + n_b1, bk.d_wsum.as<float>() + e.wsum, n_sum, hipMemcpyDeviceToHost, st), "hipMemcpyAsync(D2H)") ||
            !hip_ok(hipMemcpyAsync(o + n_img + n_b1 + n_sum, bk.d_tail.as<float>() + e.tail, n_tail, hipMemcpyDeviceToHost, st), "hipMemcpyAsync(D2H)") ||
            !hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize")) return -1;
        return 0;
    });
}

}  // extern "C"
