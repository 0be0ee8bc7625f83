// rp_train_batch.hip -- WakewordModelTrain's loop (src/wakewords/nn/wakeword_model_train.rs:204-209) for many models in one launch:
// train_batch_kernel runs one workgroup per model and a block of epochs without returning to the host.  The single-model trainer
// (launch_train_step in rp_mlp.hip) spends an epoch on 6-8 launches of kernels a few waves wide; a thousand personal models are a
// thousand independent small trainings, which fill the device when they run side by side.
//
// The bits are launch_train_step's: the build has -ffp-contract=off, so a result is decided by the order of its operations, and every
// result element is computed by one thread in that kernel's order -- sums over i / o / b ascending, never split.  The work is spread
// over result elements only (several per thread, for independent chains), rows are read four consecutive floats at a time and consumed
// in order.  Phases are separated by workgroup barriers; a model's whole state lies in its pieces of the workspace (TrainJob,
// rp_kernels.h), so a training can be cut into launches anywhere between two epochs.
// DESIGN.md §4.5.
#include "rp_mlp_dev.h"

namespace rp {

// R elements (b, o) of a layer's output, e = b * on + o = e0 + r * stride:  s = 0; for i ascending: s += x[b][i] * W[o][i];  s += bias[o]
// (mlp_layer_kernel's chain).  The R chains are independent: one thread keeps R rows in flight.
template <int R>
__device__ __forceinline__ void train_batch_dot(const float *x, const float *Wt, const float *bias, float *out, int in, int on, int relu,
                                                int e0, int stride) {
    const float *xr[R], *wr[R];
    float s[R];
    int o[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = e0 + r * stride, b = e / on;
        o[r] = e - b * on;
        xr[r] = x + (size_t)b * in;
        wr[r] = Wt + (size_t)o[r] * in;
        s[r] = 0.f;
    }
    if ((in & 3) == 0) {   // every row starts on 16 bytes (offsets are multiples of 4 floats)
        for (int i = 0; i < in; i += 4) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float4 xv = *reinterpret_cast<const float4 *>(xr[r] + i), wv = *reinterpret_cast<const float4 *>(wr[r] + i);
                s[r] += xv.x * wv.x; s[r] += xv.y * wv.y; s[r] += xv.z * wv.z; s[r] += xv.w * wv.w;
            }
        }
    } else {
        for (int i = 0; i < in; ++i) {
#pragma unroll
            for (int r = 0; r < R; ++r) s[r] += xr[r][i] * wr[r][i];
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float v = s[r] + bias[o[r]];
        if (relu && v < 0.f) v = 0.f;
        out[e0 + r * stride] = v;
    }
}

// one layer over B rows
__device__ __forceinline__ void train_batch_layer(const float *x, const float *Wt, const float *bias, float *out, int B, int in, int on, int relu) {
    const int n = B * on, T = kTrainBatchThreads;
    int e = threadIdx.x;
    for (; e + 3 * T < n; e += 4 * T) train_batch_dot<4>(x, Wt, bias, out, in, on, relu, e, T);
    for (; e < n; e += T) train_batch_dot<1>(x, Wt, bias, out, in, on, relu, e, 0);
}

// the forward over B rows, every layer's output kept in act[l]; the last layer writes `last`
__device__ __forceinline__ void train_batch_forward(const TrainJob *jb, float *ws, const float *x, int B, float *last) {
    const int nl = jb->n_layers;
    const float *cur = x;
    for (int l = 0; l < nl; ++l) {
        float *dst = l + 1 == nl ? last : ws + jb->act[l];
        train_batch_layer(cur, ws + jb->w[l], ws + jb->b[l], dst, B, jb->dims[l], jb->dims[l + 1], l + 1 < nl ? 1 : 0);
        __syncthreads();
        cur = dst;
    }
}

// train_backprop_kernel: dZprev[b][i] = A_prev[b][i] > 0 ? sum_o dZ[b][o] * W[o][i] : 0, o ascending
__device__ __forceinline__ void train_batch_backprop(const float *dz, const float *Wt, const float *a_prev, float *dz_prev, int B, int in, int on) {
    const int n = B * in;
    for (int e = threadIdx.x; e < n; e += kTrainBatchThreads) {
        const int b = e / in, i = e - b * in;
        const float *d = dz + (size_t)b * on;
        float s = 0.f;
        for (int o = 0; o < on; ++o) s += d[o] * Wt[(size_t)o * in + i];
        dz_prev[e] = a_prev[e] > 0.f ? s : 0.f;
    }
}

// train_update_kernel: W[o][i] -= lr * sum_b dZ[b][o] * A_in[b][i], bias[o] -= lr * sum_b dZ[b][o] (column i == in), b ascending.  A thread
// takes column i of four outputs: A_in[b][i] is read once for the four sums.  Outputs past `on` repeat the group's last one and are not stored.
__device__ __forceinline__ void train_batch_update(const float *dz, const float *a_in, float *Wt, float *bias, int B, int in, int on, float lr) {
    const int cols = in + 1, n = ((on + 3) / 4) * cols;
    for (int e = threadIdx.x; e < n; e += kTrainBatchThreads) {
        const int grp = e / cols, i = e - grp * cols, o0 = 4 * grp, last = on - 1;
        const int o1 = min(o0 + 1, last), o2 = min(o0 + 2, last), o3 = min(o0 + 3, last);
        float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
        if (i < in) {
            for (int b = 0; b < B; ++b) {
                const float a = a_in[(size_t)b * in + i];
                const float *d = dz + (size_t)b * on;
                g0 += d[o0] * a; g1 += d[o1] * a; g2 += d[o2] * a; g3 += d[o3] * a;
            }
            float *w = Wt + i;
            w[(size_t)o0 * in] = w[(size_t)o0 * in] - g0 * lr;
            if (o0 + 1 < on) w[(size_t)o1 * in] = w[(size_t)o1 * in] - g1 * lr;
            if (o0 + 2 < on) w[(size_t)o2 * in] = w[(size_t)o2 * in] - g2 * lr;
            if (o0 + 3 < on) w[(size_t)o3 * in] = w[(size_t)o3 * in] - g3 * lr;
        } else {
            for (int b = 0; b < B; ++b) {
                const float *d = dz + (size_t)b * on;
                g0 += d[o0]; g1 += d[o1]; g2 += d[o2]; g3 += d[o3];
            }
            bias[o0] = bias[o0] - g0 * lr;
            if (o0 + 1 < on) bias[o1] = bias[o1] - g1 * lr;
            if (o0 + 2 < on) bias[o2] = bias[o2] - g2 * lr;
            if (o0 + 3 < on) bias[o3] = bias[o3] - g3 * lr;
        }
    }
}

// One workgroup per job, the grid walks the jobs.  Per epoch: forward (a barrier behind every layer) | loss rows and dlogits | for the
// layers from the last to the first: backprop through W_l as the forward used it | barrier | update of W_l, b_l | ... | barrier.  The
// update of layer l and the backprop of layer l - 1 touch different pieces, so no barrier stands between them.
__global__ __launch_bounds__(kTrainBatchThreads) void train_batch_kernel(const TrainJob *__restrict__ jobs, int n_jobs, float *ws, float lr,
                                                                          int epochs, int test_forward) {
    for (int j = blockIdx.x; j < n_jobs; j += gridDim.x) {
        const TrainJob *jb = jobs + j;
        const int nl = jb->n_layers, B = jb->B, C = jb->dims[nl];
        const float *x = ws + jb->x;
        const int32_t *labels = reinterpret_cast<const int32_t *>(ws + jb->labels);
        float *logits = ws + jb->act[nl - 1], *dlogits = ws + jb->dz[nl - 1], *loss = ws + jb->loss;
        for (int ep = 0; ep < epochs; ++ep) {
            train_batch_forward(jb, ws, x, B, logits);
            for (int b = threadIdx.x; b < B; b += kTrainBatchThreads)
                train_softmax_row(logits + (size_t)b * C, labels[b], (size_t)B, C, dlogits + (size_t)b * C, loss + b);
            __syncthreads();
            for (int l = nl - 1; l >= 0; --l) {
                const int in = jb->dims[l], on = jb->dims[l + 1];
                if (l > 0) {
                    train_batch_backprop(ws + jb->dz[l], ws + jb->w[l], ws + jb->act[l - 1], ws + jb->dz[l - 1], B, in, on);
                    __syncthreads();
                }
                train_batch_update(ws + jb->dz[l], l == 0 ? x : ws + jb->act[l - 1], ws + jb->w[l], ws + jb->b[l], B, in, on, lr);
            }
            __syncthreads();
        }
        if (test_forward) train_batch_forward(jb, ws, ws + jb->xt, jb->Bt, ws + jb->tlog);
    }
}

hipError_t launch_train_batch(hipStream_t st, const TrainJob *jobs, size_t n_jobs, unsigned grid, float *ws, float lr, int epochs,
                              int test_forward) {
    if (n_jobs == 0 || (epochs <= 0 && !test_forward)) return hipSuccess;
    if (n_jobs > 0x7fffffffULL || grid == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(train_batch_kernel, dim3(grid), dim3(kTrainBatchThreads), 0, st, jobs, (int)n_jobs, ws, lr, epochs < 0 ? 0 : epochs,
                       test_forward);
    return hipGetLastError();
}

}  // namespace rp
