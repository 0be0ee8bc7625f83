// rp_bank_put.hip -- the device side of a wakeword bank that changes (rp_wakeword_bank_put / _put_from_rpw / _enrol, rp_bank.cpp):
// bank_put_kernel prepares template rows the way the host's prepare_template_row (rp_ctx.cpp) does, operation for operation (-ffp-contract=off:
// nothing is fused; the f64 square root and division are the correctly rounded ones), so that a wakeword put into a bank and the same
// wakeword in a bank made by rp_wakeword_bank_new give the same bits; bank_move_kernel carries the live entries of a full pool into a
// larger one.
#include "rp_device.h"

namespace rp {

constexpr int kBankPutThreads = 256;

// One lane per row of the call.  Row r belongs to the new entry e with erow[e] <= r < erow[e + 1]; its source is row esrc[e] + (r - erow[e])
// of p.src -- the staged upload of a put, or the enrolment workspace, whose templates lie in fold order while the bank holds them in the
// .rpw's order -- and it goes to row r of p.unit / p.raw (the pool tail).
__global__ __launch_bounds__(kBankPutThreads) void bank_put_kernel(BankPut p) {
    const size_t r = (size_t)blockIdx.x * kBankPutThreads + threadIdx.x;
    if (r >= p.n_rows) return;
    size_t lo = 0, hi = p.n_entries;
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if ((size_t)p.erow[mid] <= r) lo = mid; else hi = mid;
    }
    const int K = p.K;
    const float *src = p.src + ((size_t)p.esrc[lo] + (r - (size_t)p.erow[lo])) * (size_t)K;
    uint32_t *flags = p.flags + p.eww[lo];
    double nn = 0.0;
    float nf = 0.f;
    bool finite = true;
    for (int k = 0; k < K; ++k) {
        const float v = src[k];
        if (!(fabsf(v) <= 3.402823466e38f)) finite = false;
        nn += (double)v * (double)v;
    }
    if (!finite) { atomicOr(flags, kBankPutNotFinite); return; }   // the host refuses the call: nobody reads the row
    for (int k = 0; k < K; ++k) nf += src[k] * src[k];
    const double inv = (nf > 0.f && nn > 0.0) ? 1.0 / sqrt(nn) : 0.0;
    float *unit = p.unit + r * (size_t)K, *raw = p.raw + r * (size_t)K;
    for (int k = 0; k < K; ++k) {
        const float v = src[k];
        unit[k] = (float)((double)v * inv);
        raw[k] = v;
    }
    if (!(nf == 0.f || (nf >= kDtwNormLo && nf <= kDtwNormHiRow))) atomicOr(flags, kBankPutRefOnly);   // TemplatesDev::ref_only
}

hipError_t launch_bank_put(hipStream_t st, const BankPut &p) {
    if (p.n_rows == 0) return hipSuccess;
    const size_t blocks = (p.n_rows + kBankPutThreads - 1) / kBankPutThreads;
    if (p.n_entries == 0 || p.K < 1 || blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bank_put_kernel, dim3((unsigned)blocks), dim3(kBankPutThreads), 0, st, p);
    return hipGetLastError();
}

// One workgroup per live entry: its len rows of unit and raw, from row src_row of the old pool to row dst_row of the new one.
__global__ __launch_bounds__(kBankPutThreads) void bank_move_kernel(BankMove m) {
    const size_t e = blockIdx.x;
    const size_t n = (size_t)m.len[e] * (size_t)m.K, from = (size_t)m.src_row[e] * (size_t)m.K, to = (size_t)m.dst_row[e] * (size_t)m.K;
    for (size_t i = threadIdx.x; i < n; i += kBankPutThreads) {
        m.unit_new[to + i] = m.unit_old[from + i];
        m.raw_new[to + i] = m.raw_old[from + i];
    }
}

hipError_t launch_bank_move(hipStream_t st, const BankMove &m) {
    if (m.n_entries == 0) return hipSuccess;
    if (m.n_entries > 0x7fffffffULL || m.K < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bank_move_kernel, dim3((unsigned)m.n_entries), dim3(kBankPutThreads), 0, st, m);
    return hipGetLastError();
}

}  // namespace rp
