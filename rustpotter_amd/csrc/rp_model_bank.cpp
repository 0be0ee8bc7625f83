// rp_model_bank.cpp -- personal wakeword MODELS: a bank of W wakeword models resident on the device (rp_model_bank_*): model_from_data,
// ModelBank::create and the accessors.  The calls in which stream s runs ITS model are in rp_bank_calls.cpp.  The model counterpart of
// rp_bank.cpp.  DESIGN.md section 4.4.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "rp_capi.h"

using namespace rp;

namespace rp {

Model *model_from_data(Ctx *ctx, const WakewordModelData &model, int *n_layers, std::vector<int> *dims, int *none_index) {
    // init_model, src/wakewords/nn/wakeword_nn.rs:165-389: Tiny has ln1,ln2; the others ln1..ln3
    std::string mt = model.m_type;
    std::transform(mt.begin(), mt.end(), mt.begin(), ::tolower);
    *n_layers = mt == "tiny" ? 2 : (mt == "small" || mt == "medium" || mt == "large") ? 3 : 0;
    if (*n_layers == 0) { set_last_error("Unknown model type"); return nullptr; }
    dims->clear();
    std::vector<const float *> wp, bp;
    for (int l = 0; l < *n_layers; ++l) {
        auto wi = model.weights.find("ln" + std::to_string(l + 1) + ".weight");
        auto bi = model.weights.find("ln" + std::to_string(l + 1) + ".bias");
        if (wi == model.weights.end() || bi == model.weights.end() || wi->second.first.size() != 2) {
            set_last_error("Incorrect model layers");  // wakeword_nn.rs:252-256
            return nullptr;
        }
        if (l == 0) dims->push_back((int)wi->second.first[1]);
        else if ((int)wi->second.first[1] != dims->back()) { set_last_error("Incorrect model layers"); return nullptr; }
        dims->push_back((int)wi->second.first[0]);
        if (bi->second.second.size() != wi->second.first[0]) { set_last_error("Incorrect model layers"); return nullptr; }
        // the tensor must hold exactly out x in values (the dims are attacker-controlled: Model::create copies out*in floats)
        if (wi->second.first[0] == 0 || wi->second.first[1] == 0 || wi->second.first[0] > 0x7fffffffULL || wi->second.first[1] > 0x7fffffffULL ||
            wi->second.second.size() / wi->second.first[0] != wi->second.first[1] ||
            wi->second.second.size() % wi->second.first[0] != 0) { set_last_error("Incorrect model layers"); return nullptr; }
        wp.push_back(wi->second.second.data());
        bp.push_back(bi->second.second.data());
    }
    std::unique_ptr<Model> net(Model::create(ctx, *n_layers, dims->data(), wp.data(), bp.data()));
    if (!net) return nullptr;
    if (dims->back() != (int)model.labels.size()) { set_last_error("Incorrect model layers"); return nullptr; }
    *none_index = -1;
    for (size_t i = 0; i < model.labels.size(); ++i) if (model.labels[i] == "none") { *none_index = (int)i; break; }  // src/constants.rs:12
    return net.release();
}

// The bank's limits are the shapes mlp_route sends to mlp_windows_kernel: mfcc_size 16, windows of at most 256 frames, layer 1 and the tail
// layers at most 32 wide, a packed tail of at most 6144 floats.  Every refusal names its limit.
ModelBank *ModelBank::create(Ctx *ctx, size_t W, Model *const *models, int mfcc_size, const int32_t *none_index) {
    if (W > 0x7fffffffULL) { set_last_error("model bank: too many models"); return nullptr; }
    if (W && mfcc_size != 16) {
        set_last_error("model bank: mfcc_size " + std::to_string(mfcc_size) + " is not built (mlp_windows_bank_kernel takes mfcc_size 16)");
        return nullptr;
    }
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return nullptr;
    std::unique_ptr<ModelBank> b(new ModelBank());
    b->ctx = ctx;
    b->e.resize(W);
    std::vector<BankWakeword> ww(W);
    long long n_img = 0, n_b1 = 0, n_wsum = 0, n_tail = 0;
    for (size_t i = 0; i < W; ++i) {
        auto fail = [&](const std::string &why) { set_last_error("model " + std::to_string(i) + ": " + why); return nullptr; };
        if (!models[i]) return fail("null handle");
        const Model &m = *models[i];
        const MlpDev &d = m.dev;
        if (m.ctx != ctx) return fail("the model belongs to another context");
        const int nl = (int)m.dims.size() - 1;
        if (m.dims[0] % 16 != 0) return fail("an input of " + std::to_string(m.dims[0]) + " features is no whole number of frames of mfcc_size 16");
        const int L = m.dims[0] / 16;
        if (L > 256) return fail("a window of " + std::to_string(L) + " frames; the model bank takes windows of at most 256 frames");
        if (m.dims[1] > 32)
            return fail("layer 1 is " + std::to_string(m.dims[1]) + " wide; the model bank takes layer 1 at most 32 wide (every Tiny model, Small models up to 197 frames; Medium and Large models are not served from a bank)");
        for (int l = 2; l <= nl; ++l)
            if (m.dims[l] > 32) return fail("layer " + std::to_string(l) + " is " + std::to_string(m.dims[l]) + " wide; the model bank takes tail layers at most 32 wide");
        if (d.tail_floats > 6144) return fail("a packed tail of " + std::to_string(d.tail_floats) + " floats; the model bank takes at most 6144");
        if (!m.mfma_ok || !d.wwin3 || !d.b1 || !d.tail) return fail("this model has no three-part layer-1 image (mlp_windows_kernel does not take it)");
        const int ni = none_index ? none_index[i] : -1;
        if (ni < -1 || ni >= m.dims[nl]) return fail("none_index out of range");
        ModelBankEntry &e = b->e[i];
        e.wimg = n_img; e.b1 = n_b1; e.wsum = n_wsum; e.tail = n_tail;
        e.L = L; e.n1p = 16 * d.nt;
        e.n_layers = d.n_layers; e.d1 = d.dims[1]; e.d2 = d.dims[2]; e.d3 = d.dims[3];
        e.tail_floats = d.tail_floats; e.n_labels = m.dims[nl]; e.none_index = ni; e.pad = 0;
        n_img += (long long)L * 192;   // [frame][3 parts][2 k-halves][32 outputs] 16-byte pieces (MlpDev::wwin3, one 32-output tile)
        n_b1 += e.n1p; n_wsum += (long long)e.n1p * 16; n_tail += (d.tail_floats + 3) & ~3;
        b->dev.label_pitch = std::max(b->dev.label_pitch, e.n_labels);
        b->max_L = std::max(b->max_L, L);
        b->min_L = i == 0 ? L : std::min(b->min_L, L);
        // the scan's view (bank_lane): the window, an avg row, the gates already applied by nn_score_bank_kernel (>=, not >)
        ww[i] = BankWakeword{0, 0, L, 0, 0, -1.f, -1.f, 0};
    }
    b->dev.W = (int)W;
    b->scan.W = (int)W; b->scan.K = 16; b->scan.max_len = b->max_L; b->scan.min_len = b->min_L;
    if (W == 0) return b.release();
    if (!b->d_e.reserve(W * sizeof(ModelBankEntry)) || !b->d_ww.reserve(W * sizeof(BankWakeword)) || !b->d_wimg.reserve((size_t)n_img * 16) ||
        !b->d_b1.reserve((size_t)n_b1 * 4) || !b->d_wsum.reserve((size_t)n_wsum * 4) || !b->d_tail.reserve((size_t)n_tail * 4)) return nullptr;
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
        !hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) return nullptr;   // the handles may be freed when this returns
    b->dev.e = b->d_e.as<ModelBankEntry>();
    b->dev.wimg = b->d_wimg.p;
    b->dev.b1 = b->d_b1.as<float>(); b->dev.wsum = b->d_wsum.as<float>(); b->dev.tail = b->d_tail.as<float>();
    b->scan.ww = b->d_ww.as<BankWakeword>();
    return b.release();
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
        }
        return bank_handle(std::unique_ptr<ModelBank>(ModelBank::create(c, n_models, ms.data(), n_models ? K : 16, none.data())), out);
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

}  // extern "C"
