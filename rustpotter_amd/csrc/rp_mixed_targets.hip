// rp_mixed_targets.hip -- what the window and the gain normaliser of a stream come from when the stream holds wakeword references of a
// wakeword bank AND models of a model bank (mixed sets): on_wakeword_change, src/detector.rs:328-338, over every wakeword of both kinds.
#include "rp_device.h"

namespace rp {

// One side's row folded into (lmax, target, live): gain_targets_kernel's loop.  An index outside [0, W) is an empty slot.
__device__ __forceinline__ void mixed_fold(const MixedSide &m, size_t s, int &lmax, float &target, int &live) {
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

// One lane per stream.  Both rows of the stream -- references first, then models: add_wakeword's order -- are folded into
//   Lmax(s)   = the largest window over the live slots of both rows: max_len of a reference, train_size of a model
//   target(s) = the largest non-NaN level over them, NaN when none
// and written as row s of the per-stream table gain_targets_kernel writes (rp_gain_targets.hip): table[s].max_len = Lmax(s),
// level[s] = target(s), idx[s] = s, or -1 for a stream without a live slot in either row.  The per-stream gain kernels of rp_frontend.hip read it
// through PerStreamGain as they read a bank; the mixed scan kernels read Lmax(s) from it.
__global__ __launch_bounds__(64) void mixed_targets_kernel(MixedSide refs, MixedSide models, BankWakeword *__restrict__ table,
                                                           float *__restrict__ tlevel, int32_t *__restrict__ tidx, size_t S) {
    const size_t s = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (s >= S) return;
    int lmax = 0, live = 0;
    float target = __builtin_nanf("");
    mixed_fold(refs, s, lmax, target, live);
    mixed_fold(models, s, lmax, target, live);
    table[s] = BankWakeword{0, 0, lmax, -1, 0, __builtin_nanf(""), __builtin_nanf(""), 0};
    tlevel[s] = target;
    tidx[s] = live ? (int32_t)s : -1;
}

hipError_t launch_mixed_targets(hipStream_t st, const MixedSide &refs, const MixedSide &models, size_t S, void *workspace, PerStreamGain *per) {
    if (S > 0x7fffffffULL || refs.set_size < 0 || refs.set_size > 8 || models.set_size < 0 || models.set_size > 8) return hipErrorInvalidValue;
    if ((refs.set_size && !refs.rows) || (models.set_size && !models.rows)) return hipErrorInvalidValue;
    // table | level | idx, the widest element first (gain_targets_bytes)
    BankWakeword *table = static_cast<BankWakeword *>(workspace);
    float *tlevel = reinterpret_cast<float *>(table + S);
    int32_t *tidx = reinterpret_cast<int32_t *>(tlevel + S);
    per->stream_wakeword = tidx; per->ww = table; per->rms_level = tlevel; per->W = (int)S;
    if (S == 0) return hipSuccess;
    hipLaunchKernelGGL(mixed_targets_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, refs, models, table, tlevel, tidx, S);
    return hipGetLastError();
}

}  // namespace rp
