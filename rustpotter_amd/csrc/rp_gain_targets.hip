// rp_gain_targets.hip -- what the gain normaliser of a stream works towards when the stream holds SEVERAL wakewords of a bank (wakeword
// sets, model sets) or a model of a model bank: on_wakeword_change, src/detector.rs:328-338.
#include "rp_device.h"

namespace rp {

// One lane per stream.  The stream's row of set_size indices (-1, or anything outside [0, W): an empty slot) is folded into
//   Lmax(s)   = the largest max_len over the live slots                       (max_mfcc_frames, detector.rs:328-334)
//   target(s) = the largest non-NaN level over the live slots, NaN when none  (f32::max folded from NaN, detector.rs:330-333)
// and written as row s of a per-stream table in the shape PerStreamGain reads through an index: table[s].max_len = Lmax(s),
// level[s] = target(s), idx[s] = s (a stream without a live slot: -1, a detector without wakewords).  The per-stream gain kernels of
// rp_frontend.hip then take PerStreamGain{idx, table, level, W = S} as they take a bank: max(Lmax / 3, 1) and the fixed-reference rule are
// theirs.  The other fields of a table row are never read by them; they are written so that no row holds stale memory.
__global__ __launch_bounds__(64) void gain_targets_kernel(GainTargets g, size_t S) {
    const size_t s = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (s >= S) return;
    const int32_t *row = g.idx + s * (size_t)g.set_size;
    int lmax = 0, live = 0;
    float target = __builtin_nanf("");
    for (int j = 0; j < g.set_size; ++j) {
        const int wi = row[j];
        if (wi < 0 || wi >= g.W) continue;
        live = 1;
        const int len = g.ww[wi].max_len;
        lmax = len > lmax ? len : lmax;
        const float level = g.level[wi];
        // f32::max: the other operand when one is NaN
        if (!(level != level)) target = (target != target || level > target) ? level : target;
    }
    g.table[s] = BankWakeword{0, 0, lmax, -1, 0, __builtin_nanf(""), __builtin_nanf(""), 0};
    g.tlevel[s] = target;
    g.tidx[s] = live ? (int32_t)s : -1;
}

size_t gain_targets_bytes(size_t S) { return S * (sizeof(BankWakeword) + sizeof(float) + sizeof(int32_t)) + 64; }

hipError_t launch_gain_targets(hipStream_t st, const GainSource &src, const int32_t *idx, int set_size, size_t S, void *workspace,
                               PerStreamGain *per) {
    if (S > 0x7fffffffULL || set_size < 1 || set_size > 8) return hipErrorInvalidValue;   // idx[s] = s is an int32
    GainTargets g;
    g.idx = idx; g.set_size = set_size; g.ww = src.ww; g.level = src.level; g.W = src.W;
    // table | level | idx, the widest element first
    g.table = static_cast<BankWakeword *>(workspace);
    g.tlevel = reinterpret_cast<float *>(g.table + S);
    g.tidx = reinterpret_cast<int32_t *>(g.tlevel + S);
    per->stream_wakeword = g.tidx; per->ww = g.table; per->rms_level = g.tlevel; per->W = (int)S;
    if (S == 0) return hipSuccess;
    hipLaunchKernelGGL(gain_targets_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, g, S);
    return hipGetLastError();
}

}  // namespace rp
