// rp_builder.cpp -- building and saving wakeword references: WakewordRef::new_from_sample_buffers /
// new_from_sample_files (src/wakewords/comp/wakeword_ref_build.rs), MfccWavFileExtractor::compute_mfccs
// (src/mfcc/wav_file_extractor.rs:18-69), MfccAverager::average (src/mfcc/averager.rs) with the unbanded
// Dtw + back-trace (src/mfcc/dtw.rs:11-55,106-138), and WakewordSave (src/wakewords/wakeword_file.rs:10-26,
// CBOR as ciborium writes it).  rp_wakeword_ref_build: the MFCC frames come from the HIP kernel, one sample at a time, and the averaging
// is a short sequential host computation over a handful of templates (offline tooling in the reference too).  The batched forms at the
// end of the file (build_wakeword_refs, average_templates_batch) enrol many wakewords per call: one MFCC launch over all samples, the
// normalisation and the averaging on the device (rp_average.hip), bit for bit what the host code here computes.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <atomic>
#include <exception>
#include <map>
#include <thread>

#include "rp_host.h"

namespace rp {
namespace {

// ------------------------------------------------------------------------- wav
struct Wav { int channels = 0, rate = 0, bits = 0; bool is_float = false; std::vector<float> mono; };

// hound::WavReader + AudioFmt::try_from (src/mfcc/wav_file_extractor.rs:93-112) + the per-type
// Sample::into_f32 (src/audio/audio_types.rs:98-137) + first-channel mono (src/audio/encoder.rs:41-47).
// 8-bit PCM is unsigned in the file and signed (-128) in hound.
bool parse_wav(const uint8_t *b, size_t n, Wav *w, std::string *err) {
    auto u16 = [&](size_t o) { return (uint32_t)b[o] | ((uint32_t)b[o + 1] << 8); };
    auto u32 = [&](size_t o) { return u16(o) | (u16(o + 2) << 16); };
    if (n < 12 || std::memcmp(b, "RIFF", 4) != 0 || std::memcmp(b + 8, "WAVE", 4) != 0) { *err = "no RIFF tag found"; return false; }
    size_t p = 12, data_off = 0, data_len = 0;
    int fmt_tag = 0;
    bool have_fmt = false;
    while (p + 8 <= n) {
        const uint32_t sz = u32(p + 4);
        if (std::memcmp(b + p, "fmt ", 4) == 0 && p + 8 + 16 <= n) {
            fmt_tag = (int)u16(p + 8); w->channels = (int)u16(p + 10); w->rate = (int)u32(p + 12); w->bits = (int)u16(p + 22);
            if (fmt_tag == 0xFFFE && sz >= 40 && p + 8 + 26 <= n) fmt_tag = (int)u16(p + 8 + 24);  // WAVE_FORMAT_EXTENSIBLE sub-format
            have_fmt = true;
        } else if (std::memcmp(b + p, "data", 4) == 0) {
            data_off = p + 8; data_len = std::min<size_t>(sz, n - data_off);
            break;
        }
        p += 8 + (size_t)sz + (sz & 1);
    }
    if (!have_fmt || !data_off) { *err = "invalid wav file: missing fmt or data chunk"; return false; }
    w->is_float = fmt_tag == 3;
    const bool ok_fmt = (fmt_tag == 1 && (w->bits == 8 || w->bits == 16 || w->bits == 32)) || (fmt_tag == 3 && w->bits == 32);
    if (!ok_fmt || w->channels < 1) { *err = "Unsupported wav format"; return false; }  // wav_file_extractor.rs:109
    const size_t bps = (size_t)w->bits / 8, frame = bps * (size_t)w->channels, frames = data_len / frame;
    w->mono.resize(frames);
    for (size_t i = 0; i < frames; ++i) {
        const uint8_t *s = b + data_off + i * frame;  // first channel
        float v;
        if (w->is_float) { uint32_t u = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24); std::memcpy(&v, &u, 4); }
        else if (w->bits == 8) v = (float)(int8_t)(int)((int)s[0] - 128) / 127.f;
        else if (w->bits == 16) v = (float)(int16_t)((uint16_t)s[0] | ((uint16_t)s[1] << 8)) / 32767.f;
        else v = (float)(int32_t)((uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24)) / 2147483648.f;
        w->mono[i] = v;
    }
    return true;
}

// GainNormalizerFilter::get_rms_level, src/audio/gain_normalizer_filter.rs:49-55
float rms_level_of(const float *s, int n) {
    float sum_squared = 0.0f;
    for (int i = 0; i < n; ++i) sum_squared += s[i] * s[i];
    return std::sqrt(sum_squared / (float)n);
}

// the sample's level, wav_file_extractor.rs:54-58: the median RMS of the encoded buffers (0 without a whole one)
float median_chunk_rms(const std::vector<float> &mono, size_t enc_chunk) {
    std::vector<float> rms;
    for (size_t c = 0; c + enc_chunk <= (mono.size() / enc_chunk) * enc_chunk; c += enc_chunk) rms.push_back(rms_level_of(&mono[c], enc_chunk));
    if (rms.empty()) return 0.f;
    std::sort(rms.begin(), rms.end());
    return rms[rms.size() / 2];
}
// frames of an encoded sample: chunks_exact(output frame) drops a tail shorter than 30 ms, the extractor's first frame needs four shifts
size_t wav_mfcc_frames(size_t encoded_samples) {
    const size_t n = (encoded_samples / 480) * 480;
    return n >= 480 ? 3 * (n / 480) - 3 : 0;
}
// the wakeword's level: files take the median sample level (wakeword_ref_build.rs:80-81), buffers the maximum (:24-26)
float wakeword_rms_level(const std::vector<float> &levels, bool rms_median) {
    if (rms_median) { std::vector<float> s(levels); std::sort(s.begin(), s.end()); return s[s.size() / 2]; }
    float mx = 0.f;
    for (float v : levels) if (v > mx) mx = v;
    return mx;
}
// the fold order of compute_avg_samples_features (wakeword_ref_build.rs:90-110): longest template first, equal lengths by name
std::vector<size_t> fold_order(const WakewordRefData &r) {
    std::vector<size_t> order(r.tnames.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
        if (r.lens[a] != r.lens[b]) return r.lens[a] > r.lens[b];
        return r.tnames[a] < r.tnames[b];
    });
    return order;
}

// ------------------------------------------------------------------ averager
// src/mfcc/comparator.rs:15-48
float cosine_distance(const float *a, const float *b, int K) {
    float dot_ab = 0.f, dot_a = 0.f, dot_b = 0.f;
    for (int d = 0; d < K; ++d) { dot_ab += a[d] * b[d]; dot_a += a[d] * a[d]; dot_b += b[d] * b[d]; }
    const float magnitude = std::sqrt(dot_a * dot_b);
    return 1.f - (magnitude == 0.f ? 0.f : dot_ab / magnitude);
}
float min3_fold(float ins, float del, float mat) { return std::fmin(std::fmin(std::fmin(INFINITY, ins), del), mat); }

// one fold step of MfccAverager::average (src/mfcc/averager.rs:7-35): origin [m][K] <- aligned mean with frames [n][K]
void average_step(std::vector<float> &origin, int m, const std::vector<float> &frames, int n, int K) {
    std::vector<float> D((size_t)m * n);
    auto at = [&](int r, int c) -> float & { return D[(size_t)r * n + c]; };
    // Dtw::compute_optimal_path, src/mfcc/dtw.rs:11-55
    at(0, 0) = cosine_distance(&origin[0], &frames[0], K);
    for (int r = 1; r < m; ++r) at(r, 0) = cosine_distance(&origin[(size_t)r * K], &frames[0], K) + at(r - 1, 0);
    for (int c = 1; c < n; ++c) at(0, c) = cosine_distance(&origin[0], &frames[(size_t)c * K], K) + at(0, c - 1);
    for (int r = 1; r < m; ++r)
        for (int c = 1; c < n; ++c)
            at(r, c) = cosine_distance(&origin[(size_t)r * K], &frames[(size_t)c * K], K) + min3_fold(at(r - 1, c), at(r, c - 1), at(r - 1, c - 1));
    // retrieve_optimal_path, src/mfcc/dtw.rs:106-138: the vec starts with min(m-1, n-1) [0,0] entries, each move
    // pushes the NEW position (the end cell itself is never pushed), then the vec is reversed
    int r = m - 1, c = n - 1;
    std::vector<std::pair<int, int>> path((size_t)std::min(r, c), {0, 0});
    while (r > 0 || c > 0) {
        if (r > 0 && c > 0) {
            const float ins = at(r - 1, c), del = at(r, c - 1), mat = at(r - 1, c - 1), mn = min3_fold(ins, del, mat);
            if (mn == mat) { --r; --c; } else if (mn == ins) { --r; } else if (mn == del) { --c; }
        } else if (r > 0) { --r; } else { --c; }
        path.emplace_back(r, c);
    }
    std::reverse(path.begin(), path.end());
    std::vector<float> sum(origin);  // avgs[x][k] starts with origin[x][k], values appended in path order
    std::vector<int> cnt((size_t)m, 1);
    for (auto &pr : path) {
        for (int k = 0; k < K; ++k) sum[(size_t)pr.first * K + k] += frames[(size_t)pr.second * K + k];
        cnt[pr.first] += 1;
    }
    for (int x = 0; x < m; ++x)
        for (int k = 0; k < K; ++k) origin[(size_t)x * K + k] = sum[(size_t)x * K + k] / (float)cnt[x];
}

// ---------------------------------------------------------------------- CBOR
struct Cbor {
    std::vector<uint8_t> out;
    void head(int major, uint64_t v) {
        if (v < 24) out.push_back((uint8_t)((major << 5) | v));
        else if (v < 256) { out.push_back((uint8_t)((major << 5) | 24)); out.push_back((uint8_t)v); }
        else if (v < 65536) { out.push_back((uint8_t)((major << 5) | 25)); out.push_back((uint8_t)(v >> 8)); out.push_back((uint8_t)v); }
        else if (v < (1ull << 32)) { out.push_back((uint8_t)((major << 5) | 26)); for (int s = 24; s >= 0; s -= 8) out.push_back((uint8_t)(v >> s)); }
        else { out.push_back((uint8_t)((major << 5) | 27)); for (int s = 56; s >= 0; s -= 8) out.push_back((uint8_t)(v >> s)); }
    }
    void text(const std::string &s) { head(3, s.size()); out.insert(out.end(), s.begin(), s.end()); }
    void null() { out.push_back(0xf6); }
    // ciborium writes the narrowest float that round-trips (f16, else f32)
    void f32(float f) {
        uint32_t u; std::memcpy(&u, &f, 4);
        const uint32_t sign = u >> 31, exp = (u >> 23) & 0xff, man = u & 0x7fffff;
        bool half_ok = false; uint16_t h = 0;
        if (exp == 0xff) { half_ok = (man & 0x1fff) == 0; h = (uint16_t)((sign << 15) | 0x7c00 | (man >> 13)); if (man && !(man >> 13)) half_ok = false; }
        else if (exp == 0 && man == 0) { half_ok = true; h = (uint16_t)(sign << 15); }
        else {
            const int e = (int)exp - 127;
            if (e >= -14 && e <= 15 && (man & 0x1fff) == 0) { half_ok = true; h = (uint16_t)((sign << 15) | ((uint32_t)(e + 15) << 10) | (man >> 13)); }
            else if (e >= -24 && e < -14) {  // f16 subnormal
                const int shift = -14 - e;  // 1..10
                const uint32_t full = man | 0x800000;
                if ((full & ((1u << (13 + shift)) - 1)) == 0) { half_ok = true; h = (uint16_t)((sign << 15) | (full >> (13 + shift))); }
            }
        }
        if (half_ok) { out.push_back(0xf9); out.push_back((uint8_t)(h >> 8)); out.push_back((uint8_t)h); }
        else { out.push_back(0xfa); for (int s = 24; s >= 0; s -= 8) out.push_back((uint8_t)(u >> s)); }
    }
    void matrix(const std::vector<float> &m, int rows, int K) {
        head(4, (uint64_t)rows);
        for (int r = 0; r < rows; ++r) { head(4, (uint64_t)K); for (int k = 0; k < K; ++k) f32(m[(size_t)r * K + k]); }
    }
};

}  // namespace

// MfccWavFileExtractor::compute_mfccs, src/mfcc/wav_file_extractor.rs:18-69: whole-matrix-normalised MFCCs
// [frames][K] of one wav buffer + the median chunk RMS.
bool compute_wav_mfccs(Ctx *ctx, const uint8_t *buf, size_t len, int K, std::vector<float> *mfcc, int *frames, float *rms_level) {
    Wav w; std::string err;
    if (!parse_wav(buf, len, &w, &err)) { set_last_error(err); return false; }
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return false;
    // encode_samples, :71-96: chunks_exact(input frame) -> resample -> RMS of every encoded buffer -> concatenate
    size_t enc_chunk = 480;
    if (w.rate != 16000) {
        const Resampler *rs = ctx->resampler_for(w.rate);
        if (!rs) return false;
        const size_t fi = (size_t)rs->dev.fi, fo = (size_t)rs->dev.fo, nch = w.mono.size() / fi;
        std::vector<float> enc(nch * fo);
        if (nch) {
            DevBuf din, dxs, dout;
            if (!din.reserve(nch * fi * 4) || !dxs.reserve((1 + nch) * fi * 4 + 64) || !dout.reserve(nch * fo * 4)) return false;
            if (!hip_ok(hipMemcpyAsync(din.p, w.mono.data(), nch * fi * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync") ||
                !hip_ok(launch_resample_stage(ctx->stream, din.p, 3, 1, 1, nch, (int)fi, nch * fi, nullptr, dxs.as<float>()), "resample_stage_kernel") ||
                !hip_ok(launch_resample(ctx->stream, rs->dev, dxs.as<float>(), 1, nch, dout.as<float>(), nch * fo), "resample_mfma_kernel") ||
                !hip_ok(hipMemcpyAsync(enc.data(), dout.p, nch * fo * 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync") ||
                !hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"))
                return false;
        }
        w.mono.swap(enc);
        enc_chunk = fo;
    }
    if (w.mono.size() >= enc_chunk) *rms_level = median_chunk_rms(w.mono, enc_chunk);  // :54-58
    const size_t n = (w.mono.size() / 480) * 480;  // chunks_exact(output frame): a tail shorter than 30 ms is dropped
    const size_t nf = wav_mfcc_frames(w.mono.size());
    *frames = (int)nf;
    mfcc->assign(nf * K, 0.f);
    if (nf == 0) return true;
    const MfccTablesDev *tb = ctx->tables_for(K);
    if (!tb) return false;
    DevBuf dp, dm;
    if (!dp.reserve(n * 4) || !dm.reserve(nf * K * 4)) return false;
    if (!hip_ok(hipMemcpyAsync(dp.p, w.mono.data(), n * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync")) return false;
    if (!hip_ok(launch_mfcc(ctx->stream, *tb, dp.as<float>(), 1, n, n, 0, nf, nf, dm.as<float>()), "mfcc_kernel")) return false;
    std::vector<float> raw(nf * K);
    if (!hip_ok(hipMemcpyAsync(raw.data(), dm.p, nf * K * 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync")) return false;
    if (!hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) return false;
    // MfccNormalizer::normalize over the whole matrix (:67), sequential column sums
    std::vector<float> sum((size_t)K, 0.f);
    for (size_t i = 0; i < nf; ++i) for (int j = 0; j < K; ++j) sum[j] += raw[i * K + j];
    for (size_t i = 0; i < nf; ++i) for (int j = 0; j < K; ++j) (*mfcc)[i * K + j] = raw[i * K + j] - sum[j] / (float)nf;
    return true;
}

// compute_avg_samples_features, src/wakewords/comp/wakeword_ref_build.rs:90-110
static bool average_templates(const WakewordRefData &r, std::vector<float> *avg, int *avg_len) {
    const size_t T = r.tnames.size();
    if (T <= 1) return false;
    const std::vector<size_t> order = fold_order(r);
    *avg = r.feats[order[0]];
    *avg_len = r.lens[order[0]];
    for (size_t i = 1; i < T; ++i) average_step(*avg, *avg_len, r.feats[order[i]], r.lens[order[i]], r.mfcc_size);
    return true;
}

// WakewordRef::new_from_sample_buffers / _files; rms_median: files take the median sample level (:80-81),
// buffers the maximum (:24-26).
bool build_wakeword_ref(Ctx *ctx, const std::string &name, const float *threshold, const float *avg_threshold, size_t n,
                        const char *const *sample_names, const uint8_t *const *wavs, const size_t *wav_lens, int mfcc_size,
                        bool rms_median, WakewordRefData *out) {
    if (mfcc_size < 1) { set_last_error("mfcc_size must be >= 1"); return false; }
    WakewordRefData r;
    r.name = name;
    r.mfcc_size = mfcc_size;
    r.has_threshold = threshold != nullptr; r.threshold = threshold ? *threshold : 0.f;
    r.has_avg_threshold = avg_threshold != nullptr; r.avg_threshold = avg_threshold ? *avg_threshold : 0.f;
    std::vector<float> levels;
    for (size_t i = 0; i < n; ++i) {
        std::vector<float> m; int frames = 0; float level = 0.f;
        if (!compute_wav_mfccs(ctx, wavs[i], wav_lens[i], mfcc_size, &m, &frames, &level)) return false;
        if (frames == 0) { set_last_error(std::string("sample too short: ") + sample_names[i]); return false; }
        // HashMap::insert: a repeated name replaces the earlier sample
        auto it = std::find(r.tnames.begin(), r.tnames.end(), sample_names[i]);
        if (it != r.tnames.end()) { size_t k = (size_t)(it - r.tnames.begin()); r.feats[k] = std::move(m); r.lens[k] = frames; levels[k] = level; }
        else { r.tnames.push_back(sample_names[i]); r.feats.push_back(std::move(m)); r.lens.push_back(frames); levels.push_back(level); }
    }
    if (r.tnames.empty()) { set_last_error("Can not create an empty wakeword"); return false; }  // wakeword_ref.rs:52-54
    r.rms_level = wakeword_rms_level(levels, rms_median);
    r.has_avg = average_templates(r, &r.avg, &r.avg_len);
    *out = std::move(r);
    return true;
}

// WakewordSave::save_to_buffer, src/wakewords/wakeword_file.rs:22-26 (struct field order of wakeword_ref.rs:12-20)
std::vector<uint8_t> serialize_wakeword_ref(const WakewordRefData &r) {
    Cbor c;
    c.head(5, 7);
    c.text("name"); c.text(r.name);
    c.text("avg_features"); if (r.has_avg) c.matrix(r.avg, r.avg_len, r.mfcc_size); else c.null();
    c.text("samples_features"); c.head(5, r.tnames.size());
    for (size_t t = 0; t < r.tnames.size(); ++t) { c.text(r.tnames[t]); c.matrix(r.feats[t], r.lens[t], r.mfcc_size); }
    c.text("threshold"); if (r.has_threshold) c.f32(r.threshold); else c.null();
    c.text("avg_threshold"); if (r.has_avg_threshold) c.f32(r.avg_threshold); else c.null();
    c.text("rms_level"); c.f32(r.rms_level);
    c.text("mfcc_size"); c.head(0, (uint64_t)r.mfcc_size);
    return c.out;
}

// WakewordModel through WakewordSave::save_to_buffer (wakeword_model.rs:11-18, TensorData :68-72): the weight
// bytes are written as a CBOR ARRAY of small integers (serde's Vec<u8>), little-endian f32
std::vector<uint8_t> serialize_wakeword_model(const WakewordModelData &m) {
    Cbor c;
    c.head(5, 6);
    c.text("labels"); c.head(4, m.labels.size()); for (const std::string &l : m.labels) c.text(l);
    c.text("train_size"); c.head(0, (uint64_t)m.train_size);
    c.text("mfcc_size"); c.head(0, (uint64_t)m.mfcc_size);
    c.text("m_type"); c.text(m.m_type);
    c.text("weights"); c.head(5, m.weights.size());
    for (const auto &kv : m.weights) {
        c.text(kv.first);
        c.head(5, 3);
        const std::vector<float> &w = kv.second.second;
        c.text("bytes"); c.head(4, w.size() * 4);
        for (float f : w) { uint8_t b[4]; std::memcpy(b, &f, 4); for (int i = 0; i < 4; ++i) c.head(0, b[i]); }
        c.text("dims"); c.head(4, kv.second.first.size()); for (size_t d : kv.second.first) c.head(0, (uint64_t)d);
        c.text("d_type"); c.text("f32");
    }
    c.text("rms_level"); c.f32(m.rms_level);
    return c.out;
}

// ------------------------------------------------------------- batched forms
namespace {

// The averaging kernel's index arrays for W wakewords whose templates lie, in fold order, in one array of rows.
struct AvgPlan {
    size_t W = 0, nT = 0, rows = 0, avg_rows = 0;
    std::vector<int32_t> i32;   // lens [nT] | first [W] | count [W] | wakewords with the matrix in LDS [n_lds] | ... in the workspace [n_ws]
    std::vector<int64_t> i64;   // row_off [nT] | out_row [W] (-1: no average)
    size_t n_lds = 0, n_ws = 0, lds_bytes = 0, ws_lds_bytes = 0, ws_slice = 0;
    const int32_t *lens() const { return i32.data(); }
    const int32_t *first() const { return i32.data() + nT; }
    const int32_t *count() const { return i32.data() + nT + W; }
    const int64_t *row_off() const { return i64.data(); }
    const int64_t *out_row() const { return i64.data() + nT; }
};

// every_wakeword: a wakeword of one template gets rows in the output too (the caller copies that template); else only those that fold
bool plan_average(size_t W, int K, const int32_t *counts, const int32_t *lens, bool every_wakeword, AvgPlan *p) {
    size_t nT = 0;
    for (size_t w = 0; w < W; ++w) {
        if (counts[w] < 1) { set_last_error("wakeword " + std::to_string(w) + ": a wakeword needs at least one template"); return false; }
        nT += (size_t)counts[w];
    }
    if (W > 0x7fffffffULL || nT > 0x7fffffffULL) { set_last_error("too many templates for one call"); return false; }
    p->W = W; p->nT = nT;
    p->i32.assign(lens, lens + nT);
    p->i32.resize(nT + 2 * W);
    p->i64.assign(nT + W, -1);
    std::vector<int32_t> in_lds, in_ws;
    size_t t = 0;
    for (size_t w = 0; w < W; ++w) {
        const int T = counts[w], m = lens[t];
        int n_max = 1;
        for (int f = 0; f < T; ++f) {
            if (lens[t + f] < 1) { set_last_error("wakeword " + std::to_string(w) + ": a template without frames"); return false; }
            if (f) n_max = std::max(n_max, lens[t + f]);
            p->i64[t + f] = (int64_t)p->rows;
            p->rows += (size_t)lens[t + f];
        }
        p->i32[nT + w] = (int32_t)t;
        p->i32[nT + W + w] = T;
        if (T >= 2 || every_wakeword) { p->i64[nT + w] = (int64_t)p->avg_rows; p->avg_rows += (size_t)m; }
        if (T >= 2) {
            const size_t with_matrix = average_lds_bytes(m, n_max, K, true), without = average_lds_bytes(m, n_max, K, false);
            if (with_matrix <= kAvgLdsBudget) { in_lds.push_back((int32_t)w); p->lds_bytes = std::max(p->lds_bytes, with_matrix); }
            else if (without <= 160 * 1024) {
                in_ws.push_back((int32_t)w);
                p->ws_lds_bytes = std::max(p->ws_lds_bytes, without);
                p->ws_slice = std::max(p->ws_slice, average_matrix_floats(m, n_max));
            } else { set_last_error("wakeword " + std::to_string(w) + ": templates too long for the averaging kernel"); return false; }
        }
        t += (size_t)T;
    }
    p->n_lds = in_lds.size(); p->n_ws = in_ws.size();
    p->i32.insert(p->i32.end(), in_lds.begin(), in_lds.end());
    p->i32.insert(p->i32.end(), in_ws.begin(), in_ws.end());
    return true;
}

// the launches: feats [plan.rows][K] and avg [plan.avg_rows][K] on the device
bool run_average(Ctx *ctx, int K, const AvgPlan &p, const float *feats, float *avg) {
    if (p.n_lds + p.n_ws == 0) return true;
    if (!ctx->ws_enrol_i32.reserve(p.i32.size() * 4) || !ctx->ws_enrol_i64.reserve(p.i64.size() * 8)) return false;
    if (!hip_ok(hipMemcpyAsync(ctx->ws_enrol_i32.p, p.i32.data(), p.i32.size() * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync") ||
        !hip_ok(hipMemcpyAsync(ctx->ws_enrol_i64.p, p.i64.data(), p.i64.size() * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync"))
        return false;
    const int32_t *d32 = ctx->ws_enrol_i32.as<int32_t>();
    const int64_t *d64 = ctx->ws_enrol_i64.as<int64_t>();
    AverageBatch b;
    b.feats = feats; b.avg = avg; b.K = K;
    b.lens = d32; b.first = d32 + p.nT; b.count = d32 + p.nT + p.W;
    b.row_off = d64; b.out_row = d64 + p.nT;
    const int32_t *list = d32 + p.nT + 2 * p.W;
    const size_t cus = (size_t)std::max(ctx->n_cu, 1);
    if (p.n_lds && !hip_ok(launch_average(ctx->stream, b, list, p.n_lds, true, p.lds_bytes, (unsigned)std::min(p.n_lds, 2 * cus), nullptr, 0),
                           "average_kernel"))
        return false;
    if (p.n_ws) {
        // a matrix per WORKGROUP, not per wakeword; when the device cannot give that much, one workgroup takes them in turn
        size_t blocks = std::min(p.n_ws, cus);
        if (!ctx->ws_avg_matrix.reserve(blocks * p.ws_slice * 4)) {
            blocks = 1;
            if (!ctx->ws_avg_matrix.reserve(p.ws_slice * 4)) {
                set_last_error("the cost matrix of a template pair (" + std::to_string(p.ws_slice * 4) + " bytes) exceeds the workspace the context can allocate");
                return false;
            }
        }
        if (!hip_ok(launch_average(ctx->stream, b, list + p.n_lds, p.n_ws, false, p.ws_lds_bytes, (unsigned)blocks,
                                   ctx->ws_avg_matrix.as<float>(), p.ws_slice), "average_kernel (workspace)"))
            return false;
    }
    return true;
}

}  // namespace

bool average_templates_batch(Ctx *ctx, size_t W, int K, const int32_t *counts, const int32_t *lens, const float *feats, float *avg) {
    if (W == 0) return true;
    if (K < 1) { set_last_error("mfcc_size must be >= 1"); return false; }
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return false;
    AvgPlan p;
    if (!plan_average(W, K, counts, lens, true, &p)) return false;
    if (p.n_lds + p.n_ws) {
        if (!ctx->ws_enrol.reserve((p.rows + p.avg_rows) * (size_t)K * 4)) return false;
        float *d_feats = ctx->ws_enrol.as<float>(), *d_avg = d_feats + p.rows * (size_t)K;
        if (!hip_ok(hipMemcpyAsync(d_feats, feats, p.rows * (size_t)K * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync") ||
            !run_average(ctx, K, p, d_feats, d_avg) ||
            !hip_ok(hipMemcpyAsync(avg, d_avg, p.avg_rows * (size_t)K * 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync") ||
            !hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"))
            return false;
    }
    for (size_t w = 0; w < W; ++w)   // MfccAverager::average of one template: that template
        if (p.count()[w] == 1) {
            const size_t t = (size_t)p.first()[w];
            std::memcpy(avg + (size_t)p.out_row()[w] * K, feats + (size_t)p.row_off()[t] * K, (size_t)p.lens()[t] * K * 4);
        }
    return true;
}

// build_wakeword_ref for W wakewords.  What a wakeword's bytes depend on is computed as the single call computes it: the same wav
// decoding and chunk levels on the host, the same resampler pair and MFCC kernel (over all samples at once: a frame sees its own
// sample only), the same normalisation and fold, restated on the device.  enrol_front is the part up to and including the fold: it leaves
// the templates and averages in ctx->ws_enrol and everything the host knows in `out`.  Two tails take it from
// there: enrol_fetch (the copy back the .rpw writer needs) and Bank::put_rows (rp_wakeword_bank_enrol: straight into a bank, whose index
// of the call's first wakeword, first_index, the refusals count from).
bool enrol_front(Ctx *ctx, size_t W, const char *const *names, const float *thresholds, const float *avg_thresholds,
                 const size_t *counts, const char *const *sample_names, const uint8_t *const *wavs, const size_t *wav_lens,
                 int mfcc_size, bool rms_median, size_t first_index, EnrolBatch *out) {
    *out = EnrolBatch();
    if (W == 0) return true;
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return false;
    const int K = mfcc_size;
    auto refuse = [&](size_t w, const std::string &text) {
        set_last_error("wakeword " + std::to_string(first_index + w) + " (" + names[w] + "): " + text);
        return false;
    };
    // 1. every wav parsed on the host; what the single call refuses is refused here, in its order
    typedef EnrolSample Sample;
    std::vector<Sample> &smp = out->smp;
    std::vector<WakewordRefData> &refs = out->refs;
    std::vector<std::vector<size_t>> &slot_sample = out->slot_sample;   // per template slot (file order) its sample
    refs.resize(W);
    slot_sample.resize(W);
    const MfccTablesDev *tb = nullptr;
    size_t total = 0;
    for (size_t w = 0; w < W; ++w) total += counts[w];
    for (size_t g = 0; g < total; ++g)
        if (!sample_names[g] || (!wavs[g] && wav_lens[g])) { set_last_error("null argument"); return false; }
    struct Parsed { Wav wav; std::string err; bool ok = false; };
    std::vector<Parsed> parsed(total);
    parallel_for(total, [&](size_t g) { parsed[g].ok = parse_wav(wavs[g], wav_lens[g], &parsed[g].wav, &parsed[g].err); });
    for (size_t w = 0, g = 0; w < W; ++w) {
        if (!names[w]) { set_last_error("null argument"); return false; }
        if (mfcc_size < 1) return refuse(w, "mfcc_size must be >= 1");
        WakewordRefData &r = refs[w];
        r.name = names[w];
        r.mfcc_size = mfcc_size;
        r.has_threshold = thresholds && !std::isnan(thresholds[w]); r.threshold = r.has_threshold ? thresholds[w] : 0.f;
        r.has_avg_threshold = avg_thresholds && !std::isnan(avg_thresholds[w]); r.avg_threshold = r.has_avg_threshold ? avg_thresholds[w] : 0.f;
        for (size_t i = 0; i < counts[w]; ++i, ++g) {
            if (!parsed[g].ok) return refuse(w, parsed[g].err);
            Wav &wv = parsed[g].wav;
            smp.emplace_back();
            Sample &s = smp.back();
            s.mono = std::move(wv.mono);
            size_t encoded = s.mono.size();
            if (wv.rate != 16000) {
                s.rs = ctx->resampler_for(wv.rate);
                if (!s.rs) return refuse(w, std::string(last_error()));
                s.enc_chunk = (size_t)s.rs->dev.fo;
                encoded = (s.mono.size() / (size_t)s.rs->dev.fi) * (size_t)s.rs->dev.fo;
            }
            s.frames = (int)wav_mfcc_frames(encoded);
            if (s.frames == 0) return refuse(w, std::string("sample too short: ") + sample_names[g]);
            if (!tb && !(tb = ctx->tables_for(K))) return refuse(w, std::string(last_error()));
            // HashMap::insert: a repeated name replaces the earlier sample
            auto it = std::find(r.tnames.begin(), r.tnames.end(), sample_names[g]);
            if (it != r.tnames.end()) { size_t k = (size_t)(it - r.tnames.begin()); smp[slot_sample[w][k]].live = false; smp[slot_sample[w][k]].mono = {}; slot_sample[w][k] = smp.size() - 1; }
            else { r.tnames.push_back(sample_names[g]); slot_sample[w].push_back(smp.size() - 1); }
        }
        if (r.tnames.empty()) return refuse(w, "Can not create an empty wakeword");  // wakeword_ref.rs:52-54
        r.lens.resize(r.tnames.size());
        for (size_t k = 0; k < r.tnames.size(); ++k) r.lens[k] = smp[slot_sample[w][k]].frames;
    }
    std::vector<Parsed>().swap(parsed);
    // 2. samples that are not 16 kHz: the single call's resample pair, once per rate over all samples of that rate (a row per sample,
    //    padded with silence to the longest; an output frame reads its own and the previous input frame only)
    std::map<const Resampler *, std::vector<size_t>> by_rate;
    for (size_t i = 0; i < smp.size(); ++i) if (smp[i].live && smp[i].rs) by_rate[smp[i].rs].push_back(i);
    for (auto &grp : by_rate) {
        const size_t fi = (size_t)grp.first->dev.fi, fo = (size_t)grp.first->dev.fo, S = grp.second.size();
        size_t nch = 0;
        for (size_t i : grp.second) nch = std::max(nch, smp[i].mono.size() / fi);
        std::vector<float> in(S * nch * fi, 0.f), enc(S * nch * fo);
        for (size_t q = 0; q < S; ++q) { const Sample &s = smp[grp.second[q]]; std::memcpy(&in[q * nch * fi], s.mono.data(), (s.mono.size() / fi) * fi * 4); }
        DevBuf din, dxs, dout;
        if (!din.reserve(in.size() * 4) || !dxs.reserve(S * (1 + nch) * fi * 4 + 64) || !dout.reserve(enc.size() * 4)) return false;
        if (!hip_ok(hipMemcpyAsync(din.p, in.data(), in.size() * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync") ||
            !hip_ok(launch_resample_stage(ctx->stream, din.p, 3, 1, S, nch, (int)fi, nch * fi, nullptr, dxs.as<float>()), "resample_stage_kernel") ||
            !hip_ok(launch_resample(ctx->stream, grp.first->dev, dxs.as<float>(), S, nch, dout.as<float>(), nch * fo), "resample_mfma_kernel") ||
            !hip_ok(hipMemcpyAsync(enc.data(), dout.p, enc.size() * 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync") ||
            !hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"))
            return false;
        for (size_t q = 0; q < S; ++q) {
            Sample &s = smp[grp.second[q]];
            const size_t own = (s.mono.size() / fi) * fo;
            s.mono.assign(enc.begin() + q * nch * fo, enc.begin() + q * nch * fo + own);
        }
    }
    // 3. levels on the host, then ONE MFCC launch over all encoded samples, a row per sample padded to the longest
    std::vector<size_t> live;
    size_t n_max = 0;
    for (size_t i = 0; i < smp.size(); ++i) if (smp[i].live) {
        live.push_back(i);
        n_max = std::max(n_max, (smp[i].mono.size() / 480) * 480);
    }
    const size_t S = live.size(), nf_max = wav_mfcc_frames(n_max);
    // 5. (host side) name replacement is done; the templates of a wakeword lie in fold order: longest first, equal lengths by name
    std::vector<int32_t> tcounts(W), flens;
    for (size_t w = 0; w < W; ++w) {
        tcounts[w] = (int32_t)refs[w].tnames.size();
        for (size_t k : fold_order(refs[w])) flens.push_back(refs[w].lens[k]);
    }
    AvgPlan plan;
    if (!plan_average(W, K, tcounts.data(), flens.data(), false, &plan)) return false;
    for (size_t w = 0, t = 0; w < W; ++w)
        for (size_t k : fold_order(refs[w])) smp[slot_sample[w][k]].dst_row = plan.row_off()[t++];
    const size_t all_bytes = (plan.rows + plan.avg_rows) * (size_t)K * 4;
    {
        std::vector<int32_t> nf(S);
        std::vector<int64_t> dst(S);
        DevBuf &dpcm = ctx->ws_enrol_pcm, &draw = ctx->ws_enrol_raw, &dnf = ctx->ws_enrol_nf, &ddst = ctx->ws_enrol_dst;
        // the padded rows pass through page-locked memory the context keeps, a slab of at most 128 MB at a time: fresh pageable memory
        // for all rows cost more in page faults and unmapping than everything the device does in this call
        const size_t slab_rows = std::max<size_t>(1, std::min(S, ((size_t)128 << 20) / (n_max * 4)));
        if (!dpcm.reserve(S * n_max * 4) || !draw.reserve(S * nf_max * (size_t)K * 4) || !dnf.reserve(S * 4) || !ddst.reserve(S * 8) ||
            !ctx->ws_enrol.reserve(all_bytes) || !ctx->enrol_stage.reserve(slab_rows * n_max * 4))
            return false;
        float *stage = ctx->enrol_stage.as<float>();
        for (size_t q0 = 0; q0 < S; q0 += slab_rows) {
            const size_t rows = std::min(slab_rows, S - q0);
            parallel_for(rows, [&](size_t i) {   // every row is written whole by the thread that takes it
                Sample &s = smp[live[q0 + i]];
                s.level = median_chunk_rms(s.mono, s.enc_chunk);
                const size_t own = (s.mono.size() / 480) * 480;
                std::memcpy(stage + i * n_max, s.mono.data(), own * 4);
                std::memset(stage + i * n_max + own, 0, (n_max - own) * 4);
                std::vector<float>().swap(s.mono);
                nf[q0 + i] = s.frames; dst[q0 + i] = s.dst_row;
            });
            if (!hip_ok(hipMemcpyAsync(dpcm.as<float>() + q0 * n_max, stage, rows * n_max * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync") ||
                !hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"))   // the slab is free again
                return false;
        }
        float *d_tmpl = ctx->ws_enrol.as<float>(), *d_avg = d_tmpl + plan.rows * (size_t)K;
        if (!hip_ok(hipMemcpyAsync(dnf.p, nf.data(), S * 4, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync") ||
            !hip_ok(hipMemcpyAsync(ddst.p, dst.data(), S * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync") ||
            !hip_ok(launch_mfcc(ctx->stream, *tb, dpcm.as<float>(), S, n_max, n_max, 0, nf_max, nf_max, draw.as<float>()), "mfcc_kernel") ||
            // 4. MfccNormalizer::normalize over every sample's own frames, into the fold-ordered template array
            !hip_ok(launch_normalize_samples(ctx->stream, draw.as<float>(), S, nf_max, K, dnf.as<int32_t>(), ddst.as<int64_t>(), d_tmpl), "normalize_samples_kernel") ||
            // 6. the averaging kernel over all wakewords with two or more templates
            !run_average(ctx, K, plan, d_tmpl, d_avg) ||
            !hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"))   // (the index arrays above are this function's own)
            return false;
    }
    // 8. levels, and where a tail finds every wakeword's average
    out->rows = plan.rows; out->avg_rows = plan.avg_rows;
    for (size_t w = 0; w < W; ++w) {
        WakewordRefData &r = refs[w];
        std::vector<float> levels;
        for (size_t k = 0; k < r.tnames.size(); ++k) levels.push_back(smp[slot_sample[w][k]].level);
        r.rms_level = wakeword_rms_level(levels, rms_median);
        r.has_avg = plan.out_row()[w] >= 0;
        if (r.has_avg) r.avg_len = plan.lens()[plan.first()[w]];
        out->avg_row.push_back(plan.out_row()[w]);
    }
    return true;
}

// 7. one copy back of the templates and averages, and the data the writer takes
bool enrol_fetch(Ctx *ctx, int K, EnrolBatch *b) {
    if (b->refs.empty()) return true;
    std::vector<float> all((b->rows + b->avg_rows) * (size_t)K);
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice") ||
        !hip_ok(hipMemcpyAsync(all.data(), ctx->ws_enrol.p, all.size() * 4, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync") ||
        !hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"))
        return false;
    parallel_for(b->refs.size(), [&](size_t w) {
        WakewordRefData &r = b->refs[w];
        r.feats.resize(r.tnames.size());
        for (size_t k = 0; k < r.tnames.size(); ++k) {
            const EnrolSample &s = b->smp[b->slot_sample[w][k]];
            r.feats[k].assign(all.begin() + (size_t)s.dst_row * K, all.begin() + ((size_t)s.dst_row + (size_t)s.frames) * K);
        }
        if (r.has_avg) {
            const float *a = all.data() + (b->rows + (size_t)b->avg_row[w]) * K;
            r.avg.assign(a, a + (size_t)r.avg_len * K);
        }
    });
    return true;
}

bool build_wakeword_refs(Ctx *ctx, size_t W, const char *const *names, const float *thresholds, const float *avg_thresholds,
                         const size_t *counts, const char *const *sample_names, const uint8_t *const *wavs, const size_t *wav_lens,
                         int mfcc_size, bool rms_median, std::vector<WakewordRefData> *out) {
    out->clear();
    EnrolBatch b;
    if (!enrol_front(ctx, W, names, thresholds, avg_thresholds, counts, sample_names, wavs, wav_lens, mfcc_size, rms_median, 0, &b) ||
        !enrol_fetch(ctx, mfcc_size, &b))
        return false;
    *out = std::move(b.refs);
    return true;
}

std::vector<std::vector<uint8_t>> serialize_wakeword_refs(const std::vector<WakewordRefData> &refs) {
    std::vector<std::vector<uint8_t>> out(refs.size());
    parallel_for(refs.size(), [&](size_t w) { out[w] = serialize_wakeword_ref(refs[w]); });
    return out;
}

}  // namespace rp
