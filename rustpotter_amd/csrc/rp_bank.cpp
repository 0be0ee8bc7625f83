// rp_bank.cpp -- the wakeword bank object: W personal wakeword references resident on the device (rp_wakeword_bank_*): create, growth, put,
// enrol and the accessors.  The calls that score streams over a bank are in rp_bank_calls.cpp.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "rp_capi.h"

using namespace rp;

namespace rp {

Bank::~Bank() {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipFree(dev.ww); (void)hipFree(dev.tlen); (void)hipFree(dev.trow); (void)hipFree(dev.unit); (void)hipFree(dev.raw);
    (void)hipFree(rms_level);
}

bool Bank::set_rms_levels(const float *levels) {
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return false;
    if (rms_levels.empty()) return true;
    std::copy(levels, levels + rms_levels.size(), rms_levels.begin());
    // behind whatever the context's stream still runs with the old levels; the host copy is the bank's own, so it may change again at once
    return hip_ok(hipMemcpyAsync(rms_level, rms_levels.data(), rms_levels.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream),
                  "hipMemcpyAsync(rms levels)") && hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
}

template <class T> static bool upload(T **dst, const std::vector<T> &v, const char *what) {
    const size_t bytes = std::max<size_t>(v.size(), 1) * sizeof(T);   // an empty bank still owns valid pointers
    if (!hip_ok(hipMalloc(reinterpret_cast<void **>(dst), bytes), what)) return false;
    return v.empty() || hip_ok(hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice), what);
}

static std::string avg_too_long(int al, int max_len) {
    return "averaged template of " + std::to_string(al) + " frames is longer than the longest sample template (" + std::to_string(max_len) +
           " frames): a bank takes averaged templates up to the window length";
}
static std::string window_too_long(int K, int max_len) {
    const size_t fixed = ((size_t)kBankMaxTemplates * 64 + 13 * 64) * sizeof(float);
    const size_t lim = (160 * 1024 - fixed) / ((size_t)(K | 1) * sizeof(float)) - 70;
    return "wakeword template of " + std::to_string(max_len) + " frames is too long for the device kernels (limit " + std::to_string(lim) +
           " frames at mfcc_size " + std::to_string(K) + ")";
}

// What a bank refuses in wakeword w, for a new bank (ceiling, live_batches and bank_max_len 0) and for a put alike: `count` sample templates
// of lens[] frames, an averaged template of avg_len frames (0: none).  The first fault in the order below is the one reported; a call
// with faults in several wakewords names the first wakeword that has one -- that precedence is not part of the contract.
static bool wakeword_ok(size_t w, int K, long long count, const int *lens, int avg_len, int ceiling, int live_batches, int bank_max_len) {
    auto fail = [&](const std::string &why) { set_last_error("wakeword " + std::to_string(w) + ": " + why); return false; };
    if (count < 1) return fail("Can not create an empty wakeword");   // wakeword_ref.rs:53
    if (count > kBankMaxTemplates) return fail(std::to_string(count) + " templates; a bank takes at most " + std::to_string(kBankMaxTemplates) + " per wakeword");
    int ml = 0;
    for (long long t = 0; t < count; ++t) {
        if (lens[t] < 1) return fail("wakeword template without frames");
        ml = std::max(ml, lens[t]);
    }
    if (avg_len < 0) return fail("negative avg_lens");
    // dtw.rs:64-67 widens the band to |m - n| for an averaged template longer than the window; the reference's builder never makes one
    // (the average has the first sample's length) and dtw_bank_kernel is built for m == n only
    if (avg_len > ml) return fail(avg_too_long(avg_len, ml));
    if (dtw_bank_lds_bytes(K, ml) > 160 * 1024) return fail(window_too_long(K, ml));
    // a stream batch sized its MFCC history and gain ring once: the bank never comes to hold a window it has no room for
    if (ceiling && ml > ceiling) return fail("window of " + std::to_string(ml) + " frames is longer than the bank's reserved length (" + std::to_string(ceiling) + " frames, rp_wakeword_bank_reserve)");
    if (!ceiling && live_batches && ml > bank_max_len)
        return fail("window of " + std::to_string(ml) + " frames is longer than the bank's longest (" + std::to_string(bank_max_len) +
                    " frames) while a stream batch runs over the bank: call rp_wakeword_bank_reserve before creating the batch");
    return true;
}

Bank *Bank::create(Ctx *ctx, size_t W, int K, const int32_t *counts, const int32_t *lens, const float *feats, const int32_t *avg_lens,
                   const float *avg_feats, const float *thresholds, const float *avg_thresholds) {
    if (K < 1) { set_last_error("mfcc_size must be >= 1"); return nullptr; }
    if (W > 0x7fffffffULL) { set_last_error("too many wakewords"); return nullptr; }
    std::unique_ptr<Bank> bk(new Bank());
    BankDev &d = bk->dev;
    d.W = (int)W; d.K = K;
    size_t n_templates = 0, n_rows = 0, n_avg = 0, n_avg_rows = 0;
    for (size_t w = 0; w < W; ++w) {
        if (!wakeword_ok(w, K, counts[w], lens + n_templates, avg_lens ? avg_lens[w] : 0, 0, 0, 0)) return nullptr;
        for (int32_t t = 0; t < counts[w]; ++t) n_rows += (size_t)lens[n_templates + t];
        n_templates += (size_t)counts[w];
        if (avg_lens && avg_lens[w] > 0) { ++n_avg; n_avg_rows += (size_t)avg_lens[w]; }
    }
    if (n_avg && !avg_feats) { set_last_error("null argument"); return nullptr; }
    if (n_templates + n_avg > 0x7fffffffULL) { set_last_error("too many templates"); return nullptr; }
    // entries: the sample templates wakeword after wakeword, then the averaged templates; rows in the same order
    std::vector<int> tlen(n_templates + n_avg);
    std::vector<long long> trow(n_templates + n_avg);
    std::vector<float> unit((n_rows + n_avg_rows) * (size_t)K), raw((n_rows + n_avg_rows) * (size_t)K);
    bk->ww.resize(W);
    // the rows prepared as Templates::create prepares them (prepare_template_row), so that a wakeword in a bank and the same wakeword as
    // rp_templates give the same bits; false: a value is not finite
    auto put_rows = [&](const float *src, int L, size_t row0, bool *ref_only) {
        bool finite = true;
        for (int r = 0; r < L; ++r)
            finite &= prepare_template_row(src + (size_t)r * K, K, &unit[(row0 + r) * K], &raw[(row0 + r) * K], ref_only);
        return finite;
    };
    size_t e = 0, row = 0, avg_e = n_templates, avg_row = n_rows, avg_src = 0;
    d.max_len = 0; d.min_len = 0;
    for (size_t w = 0; w < W; ++w) {
        BankWakeword &bw = bk->ww[w];
        bw.first = (int)e; bw.count = counts[w]; bw.max_len = 0; bw.avg = -1; bw.ref_only = 0; bw.window_chk = 0;
        bw.threshold = thresholds ? thresholds[w] : NAN;
        bw.avg_threshold = avg_thresholds ? avg_thresholds[w] : NAN;
        bool ref_only = false, finite = true;
        for (int32_t t = 0; t < counts[w]; ++t, ++e) {
            const int L = lens[e];
            tlen[e] = L; trow[e] = (long long)row;
            finite &= put_rows(feats + row * K, L, row, &ref_only);
            row += (size_t)L;
            bw.max_len = std::max(bw.max_len, L);
        }
        const int al = avg_lens ? avg_lens[w] : 0;
        if (al > 0) {
            tlen[avg_e] = al; trow[avg_e] = (long long)avg_row;
            finite &= put_rows(avg_feats + avg_src * K, al, avg_row, &ref_only);
            bw.avg = (int)avg_e;
            ++avg_e; avg_row += (size_t)al; avg_src += (size_t)al;
        }
        if (!finite) { set_last_error("wakeword " + std::to_string(w) + ": template features must be finite"); return nullptr; }
        bw.ref_only = ref_only ? 1 : 0;
        bw.window_chk = dtw_register_staged(K, bw.max_len) ? 0 : 1;
        d.max_len = std::max(d.max_len, bw.max_len);
        d.min_len = w == 0 ? bw.max_len : std::min(d.min_len, bw.max_len);
    }
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return nullptr;
    bk->ctx = ctx;   // from here on the destructor frees what was allocated
    if (!upload(&d.ww, bk->ww, "hipMalloc(bank)") || !upload(&d.tlen, tlen, "hipMalloc(bank)") || !upload(&d.trow, trow, "hipMalloc(bank)") ||
        !upload(&d.unit, unit, "hipMalloc(bank templates)") || !upload(&d.raw, raw, "hipMalloc(bank templates)")) return nullptr;
    bk->rms_levels.assign(W, NAN);   // no reference level until rp_wakeword_bank_set_rms_levels / the .rpw files give one
    if (!upload(&bk->rms_level, bk->rms_levels, "hipMalloc(bank)")) return nullptr;
    // the pools start exactly full (see rp_host.h: a bank that grows)
    bk->n_entries = bk->cap_entries = tlen.size(); bk->n_rows = bk->cap_rows = n_rows + n_avg_rows; bk->cap_ww = W;
    bk->tlen = std::move(tlen); bk->trow = std::move(trow);
    return bk.release();
}

// ---------------------------------------------------------------------------------------------------------------- a bank that grows
bool Bank::put_check(size_t first, const std::vector<PutItem> &items) const {
    if (first > (size_t)dev.W) {
        set_last_error("first wakeword index " + std::to_string(first) + " is past the bank's " + std::to_string(dev.W) + " wakewords: a bank has no holes");
        return false;
    }
    if (items.size() > 0x7fffffffULL - first) { set_last_error("too many wakewords"); return false; }
    for (size_t i = 0; i < items.size(); ++i)
        if (!wakeword_ok(first + i, dev.K, (long long)items[i].lens.size(), items[i].lens.data(), items[i].avg_len, ceiling, live_batches, dev.max_len)) return false;
    return true;
}

template <class T> static bool dev_alloc(T **p, size_t n, const char *what) {
    return hip_ok(hipMalloc(reinterpret_cast<void **>(p), std::max<size_t>(n, 1) * sizeof(T)), what);
}

bool Bank::grow_ww(size_t cap) {
    if (cap <= cap_ww) return true;
    BankWakeword *nw = nullptr;
    float *nl = nullptr;
    const size_t W = (size_t)dev.W;
    // behind whatever still reads the old arrays; they are freed after the stream has drained
    if (!dev_alloc(&nw, cap, "hipMalloc(bank)") || !dev_alloc(&nl, cap, "hipMalloc(bank)") ||
        (W && (!hip_ok(hipMemcpyAsync(nw, dev.ww, W * sizeof(BankWakeword), hipMemcpyDeviceToDevice, ctx->stream), "hipMemcpyAsync(bank)") ||
               !hip_ok(hipMemcpyAsync(nl, rms_level, W * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream), "hipMemcpyAsync(bank)"))) ||
        !hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) {
        (void)hipFree(nw); (void)hipFree(nl);
        return false;
    }
    (void)hipFree(dev.ww); (void)hipFree(rms_level);
    dev.ww = nw; rms_level = nl; cap_ww = cap;
    return true;
}

// Growth is the compaction: the live entries, wakeword after wakeword (sample templates, then the averaged one), get consecutive places in
// the new pools; what replaced wakewords left behind stays in the old ones.
bool Bank::repool(size_t entries_cap, size_t rows_cap) {
    const size_t K = (size_t)dev.K;
    std::vector<BankWakeword> nww(ww);
    std::vector<int> ntlen;
    std::vector<long long> ntrow, from;
    size_t row = 0;
    auto take = [&](int e) {
        ntlen.push_back(tlen[(size_t)e]); from.push_back(trow[(size_t)e]); ntrow.push_back((long long)row);
        row += (size_t)tlen[(size_t)e];
        return (int)ntlen.size() - 1;
    };
    for (BankWakeword &bw : nww) {
        const int first = bw.first;
        bw.first = (int)ntlen.size();
        for (int t = 0; t < bw.count; ++t) take(first + t);
        if (bw.avg >= 0) bw.avg = take(bw.avg);
    }
    const size_t live = ntlen.size();
    if (live > entries_cap || row > rows_cap) { set_last_error("wakeword bank: pool too small for its live entries"); return false; }
    int *d_tlen = nullptr;
    long long *d_trow = nullptr;
    float *d_unit = nullptr, *d_raw = nullptr;
    auto undo = [&] { (void)hipFree(d_tlen); (void)hipFree(d_trow); (void)hipFree(d_unit); (void)hipFree(d_raw); return false; };
    if (!dev_alloc(&d_tlen, entries_cap, "hipMalloc(bank)") || !dev_alloc(&d_trow, entries_cap, "hipMalloc(bank)") ||
        !dev_alloc(&d_unit, rows_cap * K, "hipMalloc(bank templates)") || !dev_alloc(&d_raw, rows_cap * K, "hipMalloc(bank templates)"))
        return undo();
    if (live) {
        // the relocation table: from | to | len
        if (!put_ws.reserve(live * (2 * sizeof(long long) + sizeof(int32_t)))) return undo();
        long long *t_from = put_ws.as<long long>(), *t_to = t_from + live;
        int32_t *t_len = reinterpret_cast<int32_t *>(t_to + live);
        BankMove m;
        m.unit_old = dev.unit; m.raw_old = dev.raw; m.unit_new = d_unit; m.raw_new = d_raw;
        m.src_row = t_from; m.dst_row = t_to; m.len = t_len; m.n_entries = live; m.K = dev.K;
        const hipStream_t st = ctx->stream;
        if (!hip_ok(hipMemcpyAsync(t_from, from.data(), live * sizeof(long long), hipMemcpyHostToDevice, st), "hipMemcpyAsync(bank)") ||
            !hip_ok(hipMemcpyAsync(t_to, ntrow.data(), live * sizeof(long long), hipMemcpyHostToDevice, st), "hipMemcpyAsync(bank)") ||
            !hip_ok(hipMemcpyAsync(t_len, ntlen.data(), live * sizeof(int32_t), hipMemcpyHostToDevice, st), "hipMemcpyAsync(bank)") ||
            !hip_ok(launch_bank_move(st, m), "bank_move_kernel") ||
            !hip_ok(hipMemcpyAsync(d_tlen, ntlen.data(), live * sizeof(int), hipMemcpyHostToDevice, st), "hipMemcpyAsync(bank)") ||
            !hip_ok(hipMemcpyAsync(d_trow, ntrow.data(), live * sizeof(long long), hipMemcpyHostToDevice, st), "hipMemcpyAsync(bank)") ||
            !hip_ok(hipMemcpyAsync(dev.ww, nww.data(), nww.size() * sizeof(BankWakeword), hipMemcpyHostToDevice, st), "hipMemcpyAsync(bank)"))
            { (void)hipStreamSynchronize(st); return undo(); }
    }
    if (!hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) return undo();   // nothing reads the old pools any more
    (void)hipFree(dev.tlen); (void)hipFree(dev.trow); (void)hipFree(dev.unit); (void)hipFree(dev.raw);
    dev.tlen = d_tlen; dev.trow = d_trow; dev.unit = d_unit; dev.raw = d_raw;
    ww.swap(nww); tlen.swap(ntlen); trow.swap(ntrow);
    n_entries = live; n_rows = row; dead_entries = dead_rows = 0;
    cap_entries = entries_cap; cap_rows = rows_cap;
    ++grown;
    return true;
}

bool Bank::reserve(int max_len, size_t n_wakewords, size_t rows) {
    if (max_len < 0) { set_last_error("rp_wakeword_bank_reserve: max_len must be >= 0"); return false; }
    if (max_len && max_len != ceiling) {
        if (live_batches) { set_last_error("rp_wakeword_bank_reserve: the reserved length can only change while no stream batch runs over the bank"); return false; }
        if (max_len < dev.max_len) {
            set_last_error("rp_wakeword_bank_reserve: max_len " + std::to_string(max_len) + " is below the bank's longest wakeword (" + std::to_string(dev.max_len) + " frames)");
            return false;
        }
        if (dtw_bank_lds_bytes(dev.K, max_len) > 160 * 1024) { set_last_error("rp_wakeword_bank_reserve: " + window_too_long(dev.K, max_len)); return false; }
    }
    if (n_wakewords > 0x7fffffffULL) { set_last_error("too many wakewords"); return false; }
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return false;
    // hints, never limits: a wakeword has at most kBankMaxTemplates + 1 entries, so the entry pool of n_wakewords never grows again
    const size_t want_entries = std::max(cap_entries, n_wakewords * (size_t)(kBankMaxTemplates + 1)), want_rows = std::max(cap_rows, rows);
    if (!grow_ww(n_wakewords)) return false;
    if ((want_entries > cap_entries || want_rows > cap_rows) && !repool(want_entries, want_rows)) return false;
    if (max_len) ceiling = max_len;
    return true;
}

bool Bank::put_rows(size_t first, const std::vector<PutItem> &items, const float *d_src) {
    const size_t n = items.size(), K = (size_t)dev.K;
    if (n == 0) return true;
    size_t ne = 0, nr = 0;
    for (const PutItem &it : items) {
        ne += it.lens.size() + (it.avg_len > 0 ? 1 : 0);
        for (int l : it.lens) nr += (size_t)l;
        nr += (size_t)it.avg_len;
    }
    if (n_entries - dead_entries + ne > 0x7fffffffULL) { set_last_error("too many templates"); return false; }
    if (!hip_ok(hipSetDevice(ctx->device), "hipSetDevice")) return false;
    // room: a pool that is full is replaced by one at least twice its size (which drops the garbage)
    if (!grow_ww(first + n > cap_ww ? std::max(first + n, 2 * cap_ww) : cap_ww)) return false;
    const bool e_short = n_entries + ne > cap_entries, r_short = n_rows + nr > cap_rows;
    if ((e_short || r_short) &&
        !repool(e_short ? std::max(2 * cap_entries, n_entries - dead_entries + ne) : cap_entries,
                r_short ? std::max(2 * cap_rows, n_rows - dead_rows + nr) : cap_rows))
        return false;
    // the new entries, wakeword after wakeword: sample templates in the wakeword's order, then the averaged one
    std::vector<long long> tab(2 * ne + 1), ntrow(ne);   // erow [ne + 1] | esrc [ne]
    std::vector<int32_t> eww(ne);
    std::vector<int> ntlen(ne);
    std::vector<BankWakeword> nww(n);
    std::vector<float> nlevel(n);
    size_t e = 0, r = 0;
    auto entry = [&](size_t i, int len, long long src) {
        tab[e] = (long long)r; tab[ne + 1 + e] = src; eww[e] = (int32_t)i; ntlen[e] = len; ntrow[e] = (long long)(n_rows + r);
        r += (size_t)len;
        return (int)(n_entries + e++);
    };
    for (size_t i = 0; i < n; ++i) {
        const PutItem &it = items[i];
        BankWakeword &bw = nww[i];
        bw.first = (int)(n_entries + e); bw.count = (int)it.lens.size(); bw.max_len = it.max_len(); bw.avg = -1; bw.ref_only = 0;
        bw.threshold = it.threshold; bw.avg_threshold = it.avg_threshold;
        bw.window_chk = dtw_register_staged(dev.K, bw.max_len) ? 0 : 1;
        for (size_t t = 0; t < it.lens.size(); ++t) entry(i, it.lens[t], it.src[t]);
        if (it.avg_len > 0) bw.avg = entry(i, it.avg_len, it.avg_src);
        nlevel[i] = it.rms_level;
    }
    tab[ne] = (long long)nr;
    const size_t tab_bytes = tab.size() * sizeof(long long);
    if (!put_ws.reserve(tab_bytes + ne * sizeof(int32_t) + n * sizeof(uint32_t))) return false;
    BankPut p;
    p.src = d_src; p.erow = put_ws.as<long long>(); p.esrc = p.erow + ne + 1;
    int32_t *d_eww = reinterpret_cast<int32_t *>(put_ws.as<char>() + tab_bytes);
    p.eww = d_eww; p.flags = reinterpret_cast<uint32_t *>(d_eww + ne);
    p.n_entries = ne; p.n_rows = nr; p.K = dev.K;
    p.unit = dev.unit + n_rows * K; p.raw = dev.raw + n_rows * K;   // the pool tail: nothing in flight reads it
    std::vector<uint32_t> flags(n);
    const hipStream_t st = ctx->stream;
    if (!hip_ok(hipMemcpyAsync(put_ws.p, tab.data(), tab_bytes, hipMemcpyHostToDevice, st), "hipMemcpyAsync(bank)") ||
        !hip_ok(hipMemcpyAsync(d_eww, eww.data(), ne * sizeof(int32_t), hipMemcpyHostToDevice, st), "hipMemcpyAsync(bank)") ||
        !hip_ok(hipMemsetAsync(p.flags, 0, n * sizeof(uint32_t), st), "hipMemsetAsync") ||
        !hip_ok(launch_bank_put(st, p), "bank_put_kernel") ||
        !hip_ok(hipMemcpyAsync(flags.data(), p.flags, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync(bank)") ||
        !hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize"))
        return false;
    for (size_t i = 0; i < n; ++i) {
        if (flags[i] & kBankPutNotFinite) { set_last_error("wakeword " + std::to_string(first + i) + ": template features must be finite"); return false; }
        nww[i].ref_only = (flags[i] & kBankPutRefOnly) ? 1 : 0;
    }
    // commit: the entry tables' tail, then the wakewords themselves -- behind every launch that took the bank as it was
    if (!hip_ok(hipMemcpyAsync(dev.tlen + n_entries, ntlen.data(), ne * sizeof(int), hipMemcpyHostToDevice, st), "hipMemcpyAsync(bank)") ||
        !hip_ok(hipMemcpyAsync(dev.trow + n_entries, ntrow.data(), ne * sizeof(long long), hipMemcpyHostToDevice, st), "hipMemcpyAsync(bank)") ||
        !hip_ok(hipMemcpyAsync(dev.ww + first, nww.data(), n * sizeof(BankWakeword), hipMemcpyHostToDevice, st), "hipMemcpyAsync(bank)") ||
        !hip_ok(hipMemcpyAsync(rms_level + first, nlevel.data(), n * sizeof(float), hipMemcpyHostToDevice, st), "hipMemcpyAsync(bank)") ||
        !hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize"))
        return false;
    for (size_t w = first; w < std::min(first + n, ww.size()); ++w) {   // what a replaced wakeword leaves behind
        const BankWakeword &old = ww[w];
        for (int t = 0; t < old.count; ++t) dead_rows += (size_t)tlen[(size_t)(old.first + t)];
        if (old.avg >= 0) dead_rows += (size_t)tlen[(size_t)old.avg];
        dead_entries += (size_t)old.count + (old.avg >= 0 ? 1 : 0);
    }
    tlen.insert(tlen.end(), ntlen.begin(), ntlen.end());
    trow.insert(trow.end(), ntrow.begin(), ntrow.end());
    n_entries += ne; n_rows += nr;
    if (ww.size() < first + n) { ww.resize(first + n); rms_levels.resize(first + n); }
    std::copy(nww.begin(), nww.end(), ww.begin() + (long)first);
    std::copy(nlevel.begin(), nlevel.end(), rms_levels.begin() + (long)first);
    dev.W = (int)ww.size();
    dev.max_len = dev.min_len = 0;
    for (size_t w = 0; w < ww.size(); ++w) {
        dev.max_len = std::max(dev.max_len, ww[w].max_len);
        dev.min_len = w == 0 ? ww[w].max_len : std::min(dev.min_len, ww[w].max_len);
    }
    return true;
}

// the (mfcc_size, band_size) pairs the bank kernels are built for; every bank entry point refuses the others with this wording
bool bank_band_ok(const Bank &bk, int band_size) {
    const BankDev &d = bk.dev;
    if (band_size < 0) { set_last_error("band_size must be >= 0"); return false; }
    // an empty bank scores nothing (its mfcc_size is a placeholder): a Rustpotter without wakewords.  A RESERVED empty bank is a service's
    // starting state: its mfcc_size is declared, and what is enrolled later must find the kernels built
    if (d.W == 0 && !bk.ceiling) return true;
    if (band_size != 0 && dtw_register_tile(d.K, band_size) <= 0) {
        set_last_error("wakeword bank: mfcc_size " + std::to_string(d.K) + " with band_size " + std::to_string(band_size) +
                       " is not built (dtw_bank_kernel takes mfcc_size 5, 13 or 16 with band_size 3..6, or band_size 0)");
        return false;
    }
    return true;
}

bool set_size_ok(int set_size) {
    if (set_size < 1 || set_size > RP_WAKEWORD_SET_MAX) {
        set_last_error("set_size " + std::to_string(set_size) + " is outside 1 .. " + std::to_string((int)RP_WAKEWORD_SET_MAX) + " (RP_WAKEWORD_SET_MAX)");
        return false;
    }
    return true;
}

}  // namespace rp

namespace {

// W wakeword reference files in the flat layout of rp_wakeword_bank_new.  *K 0: the first file's mfcc_size is taken; every other file (all
// of them, for a *K given) must have it.  Errors name the bank index first + w.
struct RpwFlat {
    std::vector<int32_t> counts, lens, avg_lens;
    std::vector<float> feats, avg_feats, thr, athr, levels;
};
bool parse_bank_rpws(size_t first, size_t n, const uint8_t *const *rpw_buffers, const size_t *rpw_lens, int *K, RpwFlat *f) {
    for (size_t w = 0; w < n; ++w) {
        auto fail = [&](const std::string &why) { set_last_error("wakeword " + std::to_string(first + w) + ": " + why); return false; };
        if (!rpw_buffers[w]) return fail("null buffer");
        RpwKind kind;
        WakewordRefData ref;
        WakewordModelData model;
        std::string err;
        if (!parse_rpw(rpw_buffers[w], rpw_lens[w], &kind, &ref, &model, &err)) return fail(err);
        if (kind != RpwKind::Ref) return fail("a wakeword model cannot be part of a bank (wakeword references only)");
        if (*K == 0) *K = ref.mfcc_size;
        else if (ref.mfcc_size != *K) return fail("Usage of wakewords with different mfcc size is not supported, ignoring wakeword");
        f->counts.push_back((int32_t)ref.lens.size());
        for (size_t t = 0; t < ref.lens.size(); ++t) {
            f->lens.push_back(ref.lens[t]);
            f->feats.insert(f->feats.end(), ref.feats[t].begin(), ref.feats[t].end());
        }
        f->avg_lens.push_back(ref.has_avg ? ref.avg_len : 0);
        if (ref.has_avg) f->avg_feats.insert(f->avg_feats.end(), ref.avg.begin(), ref.avg.end());
        f->thr.push_back(ref.has_threshold ? ref.threshold : NAN);
        f->athr.push_back(ref.has_avg_threshold ? ref.avg_threshold : NAN);
        f->levels.push_back(ref.rms_level);
    }
    return true;
}

// rp_wakeword_bank_put and _put_from_rpw: HOST arrays in the flat layout of rp_wakeword_bank_new; the rows go to the device as they are
// (sample templates, then the averaged ones) and bank_put_kernel prepares them
int bank_put_flat(Bank &bk, size_t first, size_t n, const int32_t *counts, const int32_t *lens, const float *feats, const int32_t *avg_lens,
                  const float *avg_feats, const float *thresholds, const float *avg_thresholds, const float *rms_levels) {
    std::vector<Bank::PutItem> items(n);
    size_t t = 0, n_avg_rows = 0;
    for (size_t i = 0; i < n; ++i) {
        Bank::PutItem &it = items[i];
        for (int32_t k = 0; k < counts[i]; ++k) it.lens.push_back(lens[t++]);
        it.avg_len = avg_lens ? avg_lens[i] : 0;
        if (it.avg_len > 0) n_avg_rows += (size_t)it.avg_len;
        if (thresholds) it.threshold = thresholds[i];
        if (avg_thresholds) it.avg_threshold = avg_thresholds[i];
        if (rms_levels) it.rms_level = rms_levels[i];
    }
    if (!bk.put_check(first, items)) return -1;
    if (n_avg_rows && !avg_feats) { set_last_error("null argument"); return -1; }
    size_t rows = 0, avg_row = 0;
    for (Bank::PutItem &it : items)
        for (int l : it.lens) { it.src.push_back((long long)rows); rows += (size_t)l; }
    for (Bank::PutItem &it : items)
        if (it.avg_len > 0) { it.avg_src = (long long)(rows + avg_row); avg_row += (size_t)it.avg_len; }
    Ctx *c = bk.ctx;
    const size_t row_bytes = (size_t)bk.dev.K * sizeof(float);
    if (!hip_ok(hipSetDevice(c->device), "hipSetDevice") || !c->stage_in.reserve((rows + n_avg_rows) * row_bytes)) return -1;
    float *d = c->stage_in.as<float>();
    if (!hip_ok(hipMemcpyAsync(d, feats, rows * row_bytes, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync(H2D)") ||
        (n_avg_rows && !hip_ok(hipMemcpyAsync(d + rows * (size_t)bk.dev.K, avg_feats, n_avg_rows * row_bytes, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync(H2D)")))
        return -1;
    return bk.put_rows(first, items, d) ? 0 : -1;
}

int bank_from(rp_ctx *ctx, std::unique_ptr<Bank> b, rp_wakeword_bank **out) {
    (void)ctx;
    if (!b) return -1;
    rp_wakeword_bank *h = new rp_wakeword_bank();
    h->impl = std::move(b);
    *out = h;
    return 0;
}

}  // namespace

extern "C" {

static_assert(RP_DTW_KERNEL_BANK_SETS == (int)kDtwRanBankSets && RP_DTW_KERNEL_BANK_SETS_STREAM == (int)kDtwRanBankSetsStream && RP_WAKEWORD_SET_MAX == kScanMaxWakewords, "rustpotter_hip.h mirrors rp_kernels.h");
static_assert(RP_DTW_KERNEL_MIXED_SETS_STREAM == (int)kDtwRanMixedSetsStream, "rustpotter_hip.h mirrors rp_kernels.h");
static_assert(RP_DTW_KERNEL_BANK == (int)kDtwRanBank && RP_DTW_KERNEL_BANK_STREAM == (int)kDtwRanBankStream && RP_WAKEWORD_BANK_MAX_TEMPLATES == kBankMaxTemplates, "rustpotter_hip.h mirrors rp_kernels.h");

int rp_wakeword_bank_new(rp_ctx *ctx, size_t n_wakewords, int mfcc_size, const int32_t *counts, const int32_t *lens, const float *feats,
                         const int32_t *avg_lens, const float *avg_feats, const float *thresholds, const float *avg_thresholds,
                         rp_wakeword_bank **out) {
    return guarded([&]() -> int {
        if (!ctx || !out) { set_last_error("null argument"); return -1; }
        *out = nullptr;
        if (n_wakewords && (!counts || !lens || !feats)) { set_last_error("null argument"); return -1; }
        return bank_from(ctx, std::unique_ptr<Bank>(Bank::create(ctx->impl.get(), n_wakewords, mfcc_size, counts, lens, feats, avg_lens, avg_feats,
                                                                 thresholds, avg_thresholds)), out);
    });
}

int rp_wakeword_bank_new_from_rpw(rp_ctx *ctx, size_t n_wakewords, const uint8_t *const *rpw_buffers, const size_t *rpw_lens,
                                  rp_wakeword_bank **out) {
    return guarded([&]() -> int {
        if (!ctx || !out) { set_last_error("null argument"); return -1; }
        *out = nullptr;
        if (n_wakewords && (!rpw_buffers || !rpw_lens)) { set_last_error("null argument"); return -1; }
        RpwFlat f;
        int K = 0;
        if (!parse_bank_rpws(0, n_wakewords, rpw_buffers, rpw_lens, &K, &f)) return -1;
        if (n_wakewords == 0) K = 1;
        std::unique_ptr<Bank> bk(Bank::create(ctx->impl.get(), n_wakewords, K, f.counts.data(), f.lens.data(), f.feats.data(), f.avg_lens.data(),
                                              f.avg_feats.data(), f.thr.data(), f.athr.data()));
        if (bk && !bk->set_rms_levels(f.levels.data())) return -1;
        return bank_from(ctx, std::move(bk), out);
    });
}

int rp_wakeword_bank_set_rms_levels(rp_wakeword_bank *bank, const float *rms_levels) {
    return guarded([&]() -> int {
        if (!bank) { set_last_error("null handle"); return -1; }
        if (!rms_levels && bank->impl->dev.W) { set_last_error("null argument"); return -1; }
        return bank->impl->set_rms_levels(rms_levels) ? 0 : -1;
    });
}

float rp_wakeword_bank_rms_level(const rp_wakeword_bank *bank, long long wakeword) {
    if (!bank || wakeword < 0 || wakeword >= (long long)bank->impl->dev.W) return NAN;
    return bank->impl->rms_levels[(size_t)wakeword];
}

void rp_wakeword_bank_free(rp_wakeword_bank *bank) { delete bank; }

int rp_wakeword_bank_size(const rp_wakeword_bank *bank) {
    if (!bank) { set_last_error("null handle"); return -1; }
    return bank->impl->dev.W;
}

int rp_wakeword_bank_reserved_len(const rp_wakeword_bank *bank) {
    if (!bank) { set_last_error("null handle"); return -1; }
    return bank->impl->ceiling;
}

int rp_wakeword_bank_pool_growths(const rp_wakeword_bank *bank) {
    if (!bank) { set_last_error("null handle"); return -1; }
    return (int)std::min<size_t>(bank->impl->grown, 0x7fffffff);
}

int rp_wakeword_bank_reserve(rp_wakeword_bank *bank, int max_len, size_t n_wakewords, size_t n_rows) {
    return guarded([&]() -> int {
        if (!bank) { set_last_error("null handle"); return -1; }
        return bank->impl->reserve(max_len, n_wakewords, n_rows) ? 0 : -1;
    });
}

int rp_wakeword_bank_put(rp_wakeword_bank *bank, size_t first, size_t n, const int32_t *counts, const int32_t *lens, const float *feats,
                         const int32_t *avg_lens, const float *avg_feats, const float *thresholds, const float *avg_thresholds,
                         const float *rms_levels) {
    return guarded([&]() -> int {
        if (!bank) { set_last_error("null handle"); return -1; }
        if (n == 0) return 0;
        if (!counts || !lens || !feats) { set_last_error("null argument"); return -1; }
        return bank_put_flat(*bank->impl, first, n, counts, lens, feats, avg_lens, avg_feats, thresholds, avg_thresholds, rms_levels);
    });
}

int rp_wakeword_bank_put_from_rpw(rp_wakeword_bank *bank, size_t first, size_t n, const uint8_t *const *rpw_buffers, const size_t *rpw_lens) {
    return guarded([&]() -> int {
        if (!bank) { set_last_error("null handle"); return -1; }
        if (n == 0) return 0;
        if (!rpw_buffers || !rpw_lens) { set_last_error("null argument"); return -1; }
        Bank &bk = *bank->impl;
        // an empty bank nobody has declared a size for (no reserve, no batch) takes the files' mfcc_size, as rp_wakeword_bank_new_from_rpw does
        const bool adopt = bk.dev.W == 0 && !bk.ceiling && !bk.live_batches;
        const int K_was = bk.dev.K;
        RpwFlat f;
        int K = adopt ? 0 : K_was;
        if (!parse_bank_rpws(first, n, rpw_buffers, rpw_lens, &K, &f)) return -1;
        bk.dev.K = K;
        const int r = bank_put_flat(bk, first, n, f.counts.data(), f.lens.data(), f.feats.data(), f.avg_lens.data(), f.avg_feats.data(), f.thr.data(),
                                    f.athr.data(), f.levels.data());
        if (r != 0) bk.dev.K = K_was;   // a refused call leaves the bank as it was
        return r;
    });
}

int rp_wakeword_bank_enrol(rp_wakeword_bank *bank, size_t first, size_t n, const char *const *names, const float *thresholds,
                           const float *avg_thresholds, const size_t *counts, const char *const *sample_names,
                           const uint8_t *const *wav_buffers, const size_t *wav_lens, int rms_from_files, uint8_t **out_rpw, size_t *out_lens) {
    return guarded([&]() -> int {
        if (!bank) { set_last_error("null handle"); return -1; }
        if ((out_rpw != nullptr) != (out_lens != nullptr)) { set_last_error("null argument"); return -1; }
        if (n && (!names || !counts)) { set_last_error("null argument"); return -1; }
        size_t total = 0;
        for (size_t w = 0; w < n; ++w) { if (out_rpw) { out_rpw[w] = nullptr; out_lens[w] = 0; } total += counts[w]; }
        if (total && (!sample_names || !wav_buffers || !wav_lens)) { set_last_error("null argument"); return -1; }
        if (n == 0) return 0;
        Bank &bk = *bank->impl;
        Ctx *c = bk.ctx;
        const int K = bk.dev.K;
        if (!bk.put_check(first, {})) return -1;   // `first` alone, before the work of an enrolment
        // rp_wakeword_ref_build_batch up to and including the fold; its refusals name the wakeword by its bank index
        EnrolBatch eb;
        if (!enrol_front(c, n, names, thresholds, avg_thresholds, counts, sample_names, wav_buffers, wav_lens, K, rms_from_files != 0, first, &eb)) return -1;
        // the templates as the .rpw lists them (file order), read from where the fold order put them
        std::vector<Bank::PutItem> items(n);
        for (size_t w = 0; w < n; ++w) {
            const WakewordRefData &r = eb.refs[w];
            Bank::PutItem &it = items[w];
            for (size_t k = 0; k < r.tnames.size(); ++k) {
                const EnrolSample &sm = eb.smp[eb.slot_sample[w][k]];
                it.lens.push_back(sm.frames);
                it.src.push_back((long long)sm.dst_row);
            }
            if (r.has_avg) { it.avg_len = r.avg_len; it.avg_src = (long long)(eb.rows + (size_t)eb.avg_row[w]); }
            it.threshold = r.has_threshold ? r.threshold : NAN;
            it.avg_threshold = r.has_avg_threshold ? r.avg_threshold : NAN;
            it.rms_level = r.rms_level;
        }
        if (!bk.put_check(first, items)) return -1;
        // the files, when asked for: exactly rp_wakeword_ref_build_batch's tail, finished before the bank changes
        std::vector<std::vector<uint8_t>> bytes;
        if (out_rpw) {
            if (!enrol_fetch(c, K, &eb)) return -1;
            bytes = serialize_wakeword_refs(eb.refs);
        }
        auto drop = [&] { for (size_t w = 0; out_rpw && w < n; ++w) { std::free(out_rpw[w]); out_rpw[w] = nullptr; out_lens[w] = 0; } return -1; };
        for (size_t w = 0; out_rpw && w < n; ++w) {
            out_rpw[w] = static_cast<uint8_t *>(std::malloc(std::max<size_t>(bytes[w].size(), 1)));
            if (!out_rpw[w]) { set_last_error("out of host memory"); return drop(); }
            std::memcpy(out_rpw[w], bytes[w].data(), bytes[w].size());
            out_lens[w] = bytes[w].size();
        }
        if (!bk.put_rows(first, items, c->ws_enrol.as<float>())) return drop();
        return 0;
    });
}

int rp_wakeword_bank_max_len(const rp_wakeword_bank *bank, long long wakeword) {
    if (!bank) { set_last_error("null handle"); return -1; }
    const Bank &b = *bank->impl;
    if (wakeword < 0) return b.dev.max_len;
    if (wakeword >= (long long)b.dev.W) { set_last_error("wakeword index outside the bank"); return -1; }
    return b.ww[(size_t)wakeword].max_len;
}

}  // extern "C"
