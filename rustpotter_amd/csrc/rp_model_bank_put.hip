// rp_model_bank_put.hip -- the device side of a model bank that changes (rp_model_bank_put / _put_from_rpw / _train, rp_model_bank.cpp):
// model_bank_put_kernel builds the four pool entries of every model of a call from its raw f32 parameters the way the host does in
// Model::create, Model::wsum_for(16) and ModelBank::create, operation for operation (-ffp-contract=off: nothing is fused; f32 denormals are
// kept), so that a model put into a bank and the same model in a bank made by rp_model_bank_new give the same bits; model_bank_move_kernel
// carries the live models of a full pool into a larger one.
#include "rp_device.h"

namespace rp {

constexpr int kModelPutThreads = 256;
constexpr int kModelPutFrames = 4;      // frames of layer 1 a workgroup turns into pieces: 256 bytes = two whole lines of every weight row
constexpr int kModelPutRowPitch = 68;   // floats between the staged rows: lanes 4 j words apart read their 16 bytes without a bank conflict

__device__ __forceinline__ uint32_t put_bf16_rtn(float v) {   // bf16_rtn_bits
    uint32_t u = __float_as_uint(v);
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}
__device__ __forceinline__ float put_bf16_f32(uint32_t b) { return __uint_as_float(b << 16); }
__device__ __forceinline__ bool put_finite(float v) { return fabsf(v) <= 3.402823466e38f; }

// bf16_split3 of rp_ctx.cpp: a = p0 + p1 + p2, rounded to nearest; truncated where a rounding carried a part out of reach
__device__ __forceinline__ void put_split3(float a, uint32_t p[3]) {
    p[0] = put_bf16_rtn(a);
    const float r1 = a - put_bf16_f32(p[0]);
    p[1] = put_bf16_rtn(r1);
    const float r2 = r1 - put_bf16_f32(p[1]);
    p[2] = put_bf16_rtn(r2);
    if (put_bf16_f32(p[0]) + put_bf16_f32(p[1]) + put_bf16_f32(p[2]) != a) {
        p[0] = __float_as_uint(a) >> 16;
        const float t1 = a - put_bf16_f32(p[0]);
        p[1] = __float_as_uint(t1) >> 16;
        const float t2 = t1 - put_bf16_f32(p[1]);
        p[2] = __float_as_uint(t2) >> 16;
    }
}

// the workgroups a model of window L, n1p rows and a tail pitch of tp floats needs: image groups | wsum | b1 and tail
__host__ __device__ inline int put_img_units(int L) { return (L + kModelPutFrames - 1) / kModelPutFrames; }
__host__ __device__ inline int put_sum_units(int n1p) { return n1p * 16 / kModelPutThreads; }
__host__ __device__ inline int put_tail_units(int n1p, int tp) { return (n1p + tp + kModelPutThreads - 1) / kModelPutThreads; }

// `units` workgroups per model, the call's largest; a model with less work leaves the others idle.
//   image: frames 4 g .. 4 g + 3.  Lane t stages the 8 weights W1[t / 8][16 (4 g) + 8 (t % 8) ..] -- 8 lanes read the 256 contiguous bytes
//   of a row -- then lane (fl, h, j = t % 32) splits its 8 values and writes the three pieces, 32 lanes 512 contiguous bytes each.
//   wsum: lane (o, k) walks the frames.  b1 / tail: a lane per float.
__global__ __launch_bounds__(kModelPutThreads) void model_bank_put_kernel(ModelBankPut p, int units) {
    __shared__ __attribute__((aligned(16))) float stage[32 * kModelPutRowPitch];
    const size_t i = blockIdx.x / (unsigned)units;
    int u = (int)(blockIdx.x % (unsigned)units);
    const int t = threadIdx.x;
    const ModelPutItem &it = p.items[i];
    const ModelBankEntry e = it.e;
    const int L = e.L, d1 = e.d1, n1p = e.n1p, in = 16 * L;
    const int tail_pitch = (e.tail_floats + 3) & ~3;
    const float *w1 = it.w[0];
    bool finite = true;
    const int G = put_img_units(L), S = put_sum_units(n1p);
    if (u < G) {
        const int f0 = u * kModelPutFrames;
        {
            const int j = t >> 3, c = t & 7, f = f0 + (c >> 1);
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
            if (j < d1 && f < L) {
                const f32x4 *src = reinterpret_cast<const f32x4 *>(w1 + (size_t)j * in + 16 * f0 + 8 * c);
                a = src[0]; b = src[1];
                for (int q = 0; q < 4; ++q) finite = finite && put_finite(a[q]) && put_finite(b[q]);
            }
            f32x4 *dst = reinterpret_cast<f32x4 *>(stage + j * kModelPutRowPitch + 8 * c);
            dst[0] = a; dst[1] = b;
        }
        __syncthreads();
        const int j = t & 31, h = (t >> 5) & 1, fl = t >> 6, f = f0 + fl;
        if (f < L) {
            const f32x4 *src = reinterpret_cast<const f32x4 *>(stage + j * kModelPutRowPitch + 16 * fl + 8 * h);
            const f32x4 a = src[0], b = src[1];
            uint32_t part[3][4];
            for (int q = 0; q < 4; ++q) {
                uint32_t lo[3], hi[3];
                const float v0 = q < 2 ? a[2 * q] : b[2 * q - 4], v1 = q < 2 ? a[2 * q + 1] : b[2 * q - 3];
                put_split3(v0, lo);
                put_split3(v1, hi);
                for (int k = 0; k < 3; ++k) part[k][q] = (lo[k] & 0xffffu) | (hi[k] << 16);
            }
            uint4 *img = static_cast<uint4 *>(p.wimg) + e.wimg;
            for (int k = 0; k < 3; ++k)
                img[(((size_t)f * 3 + k) * 2 + h) * 32 + j] = make_uint4(part[k][0], part[k][1], part[k][2], part[k][3]);
        }
    } else if ((u -= G) < S) {
        const int idx = u * kModelPutThreads + t, o = idx >> 4, k = idx & 15;
        if (o < n1p) {
            double acc = 0.0;
            if (o < d1)
                for (int f = 0; f < L; ++f) acc += (double)w1[(size_t)o * in + 16 * f + k];
            p.wsum[e.wsum + idx] = (float)acc;
        }
    } else if ((u -= S) < put_tail_units(n1p, tail_pitch)) {
        const int idx = u * kModelPutThreads + t;
        if (idx < n1p) {
            const float v = idx < d1 ? it.b[0][idx] : 0.f;
            finite = put_finite(v);
            p.b1[e.b1 + idx] = v;
        } else if (idx - n1p < tail_pitch) {
            // layers 2..: weights [out][in] then bias [out] per layer; a model without a tail layer holds one 0.f; zeros up to the pitch
            int q = idx - n1p;
            float v = 0.f;
            if (q < e.tail_floats && e.n_layers >= 2) {
                const int n2 = e.d2 * d1;
                if (q < n2) v = it.w[1][q];
                else if ((q -= n2) < e.d2) v = it.b[1][q];
                else if (e.n_layers >= 3) {
                    const int n3 = e.d3 * e.d2;
                    q -= e.d2;
                    v = q < n3 ? it.w[2][q] : it.b[2][q - n3];
                }
            }
            finite = put_finite(v);
            p.tail[e.tail + (idx - n1p)] = v;
        }
    }
    if (!finite) atomicOr(p.flags + i, kModelPutNotFinite);   // the host refuses the call: nobody reads the entries
}

hipError_t launch_model_bank_put(hipStream_t st, const ModelBankPut &p) {
    if (p.n == 0) return hipSuccess;
    if (p.max_L < 1 || p.max_L > 256 || p.max_tail < 0) return hipErrorInvalidValue;
    const int units = put_img_units(p.max_L) + put_sum_units(32) + put_tail_units(32, p.max_tail);
    if (p.n > 0x7fffffffULL / (size_t)units) return hipErrorInvalidValue;
    hipLaunchKernelGGL(model_bank_put_kernel, dim3((unsigned)(p.n * (size_t)units)), dim3(kModelPutThreads), 0, st, p, units);
    return hipGetLastError();
}

// One workgroup per live model: its image pieces, b1, wsum and tail from their places in the old pools to those in the new.
__global__ __launch_bounds__(kModelPutThreads) void model_bank_move_kernel(ModelBankMove m) {
    const ModelBankEntry a = m.from[blockIdx.x], b = m.to[blockIdx.x];
    const uint4 *io = static_cast<const uint4 *>(m.wimg_old) + a.wimg;
    uint4 *in = static_cast<uint4 *>(m.wimg_new) + b.wimg;
    const int n_img = a.L * 192, n_sum = a.n1p * 16;
    for (int i = threadIdx.x; i < n_img; i += kModelPutThreads) in[i] = io[i];
    for (int i = threadIdx.x; i < a.n1p; i += kModelPutThreads) m.b1_new[b.b1 + i] = m.b1_old[a.b1 + i];
    for (int i = threadIdx.x; i < n_sum; i += kModelPutThreads) m.wsum_new[b.wsum + i] = m.wsum_old[a.wsum + i];
    for (int i = threadIdx.x; i < a.tail_floats; i += kModelPutThreads) m.tail_new[b.tail + i] = m.tail_old[a.tail + i];
}

hipError_t launch_model_bank_move(hipStream_t st, const ModelBankMove &m) {
    if (m.n == 0) return hipSuccess;
    if (m.n > 0x7fffffffULL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(model_bank_move_kernel, dim3((unsigned)m.n), dim3(kModelPutThreads), 0, st, m);
    return hipGetLastError();
}

}  // namespace rp
