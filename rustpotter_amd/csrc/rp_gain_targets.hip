// rp_gain_targets.hip -- what the window and the gain normaliser of a stream come from when the stream holds SEVERAL entries of a bank
// (wakeword sets, model sets), a model of a model bank, or wakeword references AND models of two banks (mixed sets): on_wakeword_change,
// src/detector.rs:328-338, over every wakeword the stream holds.
#include "rp_device.h"

namespace rp {

// One side's row folded into (lmax, target, live).  An index outside [0, W) is an empty slot.
__device__ __forceinline__ void targets_fold(const TargetSide &m, size_t s, int &lmax, float &target, int &live) {
    const int32_t *row = m.rows + s * (size_t)m.set_size;
    for (int j = 0; j < m.set_size; ++j) {
        const int wi = row[j];
        if (wi < 0 || wi >= m.W) continue;
        live = 1;
        const int len = m.ww[wi].max_len;
        lmax = len > lmax ? len : lmax;
        const float level = m.level[wi];
        // f32::max: the other operand when one is NaN
        if (!(level != level)) target = (target != target || level > target) ? level : target;
    }
}

// One lane per stream.  The stream's rows -- references first, then models: add_wakeword's order -- are folded into
//   Lmax(s)   = the largest window over the live slots: max_len of a reference, train_size of a model  (max_mfcc_frames, detector.rs:328-334)
//   target(s) = the largest non-NaN level over them, NaN when none                                     (f32::max folded from NaN, :330-333)
// and written as row s of a per-stream table in the shape PerStreamGain reads through an index: table[s].max_len = Lmax(s),
// level[s] = target(s), idx[s] = s (a stream without a live slot: -1, a detector without wakewords).  The per-stream gain kernels of
// rp_frontend.hip then take PerStreamGain{idx, table, level, W = S} as they take a bank: max(Lmax / 3, 1) and the fixed-reference rule are
// theirs.  The other fields of a table row are never read by them; they are written so that no row holds stale memory.
__global__ __launch_bounds__(64) void stream_targets_kernel(TargetSide first, TargetSide second, BankWakeword *__restrict__ table,
                                                            float *__restrict__ tlevel, int32_t *__restrict__ tidx, size_t S) {
    const size_t s = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (s >= S) return;
    int lmax = 0, live = 0;
    float target = __builtin_nanf("");
    targets_fold(first, s, lmax, target, live);
    targets_fold(second, s, lmax, target, live);
    table[s] = BankWakeword{0, 0, lmax, -1, 0, __builtin_nanf(""), __builtin_nanf(""), 0};
    tlevel[s] = target;
    tidx[s] = live ? (int32_t)s : -1;
}

size_t gain_targets_bytes(size_t S) { return S * (sizeof(BankWakeword) + sizeof(float) + sizeof(int32_t)) + 64; }

hipError_t launch_stream_targets(hipStream_t st, const TargetSide &first, const TargetSide &second, size_t S, void *workspace, PerStreamGain *per) {
    if (S > 0x7fffffffULL) return hipErrorInvalidValue;   // idx[s] = s is an int32
    for (const TargetSide *m : {&first, &second})
        if (m->set_size < 0 || m->set_size > 8 || (m->set_size && !m->rows)) return hipErrorInvalidValue;
    // table | level | idx, the widest element first
    BankWakeword *table = static_cast<BankWakeword *>(workspace);
    float *tlevel = reinterpret_cast<float *>(table + S);
    int32_t *tidx = reinterpret_cast<int32_t *>(tlevel + S);
    per->stream_wakeword = tidx; per->ww = table; per->rms_level = tlevel; per->W = (int)S;
    if (S == 0) return hipSuccess;
    hipLaunchKernelGGL(stream_targets_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, first, second, table, tlevel, tidx, S);
    return hipGetLastError();
}

}  // namespace rp
