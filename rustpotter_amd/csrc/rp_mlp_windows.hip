// rp_mlp_windows.hip -- the wakeword-model forward over ALL windows of a stream from one staging of its frames: mlp_windows_kernel,
// mlp_windows_wide_kernel, mlp_windows_bank_kernel (per-stream models of a bank) and the window means they correct with.  Their shared
// pieces are in rp_mlp_dev.h; mlp_route (rp_mlp.hip) decides when they run.  DESIGN.md §4.4.
#include "rp_mlp_windows.h"
#include "rp_host.h"

namespace rp {

// (window_means_body, the sums of every window-means kernel, is in rp_mlp_dev.h: rp_mlp_bank_stream.hip shares it)
__global__ __launch_bounds__(256) void window_means_kernel(const float *__restrict__ mfcc, size_t n_frames, size_t n_win, unsigned tiles,
                                                           int L, int K, float *__restrict__ mean) {
    const size_t s = blockIdx.x / tiles;
    const size_t w0 = (size_t)(blockIdx.x - s * tiles) * 64;
    const size_t nw = n_win - w0 < 64 ? n_win - w0 : 64;
    window_means_body(mfcc + (s * n_frames + w0) * K, (int)nw, L, K, mean + (s * n_win + w0) * K);
}

hipError_t launch_window_means(hipStream_t st, const float *mfcc, size_t S, size_t n_frames, size_t n_win, int L, int K, float *mean) {
    if (S == 0 || n_win == 0) return hipSuccess;
    const size_t tiles = (n_win + 63) / 64, blocks = tiles * S;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    const size_t lds = (size_t)(64 + L - 1) * K * sizeof(float);
    if (lds > 64 * 1024 || K % 4 != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(window_means_kernel, dim3((unsigned)blocks), dim3(256), lds, st, mfcc, n_frames, n_win, (unsigned)tiles, L, K, mean);
    return hipGetLastError();
}

// the same with every stream's own window length (mfcc_size 16, a constant here): the same sums in frame order, hence the same bits;
// blocks behind a stream's windows leave
__global__ __launch_bounds__(256) void window_means_bank_kernel(ModelBankDev b, const int32_t *__restrict__ stream_model, const float *__restrict__ mfcc,
                                                                size_t n_frames, unsigned tiles, size_t win_pitch, float *__restrict__ mean) {
    const size_t s = blockIdx.x / tiles;
    const size_t w0 = (size_t)(blockIdx.x - s * tiles) * 64;
    const int mi = stream_model[s];
    if (mi < 0 || mi >= b.W) return;
    const int L = b.e[mi].L;
    if (n_frames < (size_t)L) return;
    const size_t n_win = n_frames - (size_t)L + 1;
    if (w0 >= n_win) return;
    const size_t nw = n_win - w0 < 64 ? n_win - w0 : 64;
    window_means_body(mfcc + (s * n_frames + w0) * 16, (int)nw, L, 16, mean + (s * win_pitch + w0) * 16);
}

hipError_t launch_window_means_bank(hipStream_t st, const ModelBankDev &b, const int32_t *stream_model, const float *mfcc, size_t S, size_t n_frames,
                                    size_t win_pitch, float *mean) {
    if (S == 0 || win_pitch == 0 || b.W == 0) return hipSuccess;
    const size_t tiles = (win_pitch + 63) / 64, blocks = tiles * S;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    const size_t lds = (size_t)(64 + 256 - 1) * 16 * sizeof(float);   // the bank's longest window: 256 frames
    hipLaunchKernelGGL(window_means_bank_kernel, dim3((unsigned)blocks), dim3(256), lds, st, b, stream_model, mfcc, n_frames, (unsigned)tiles, win_pitch,
                       mean);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------
// Layer 1 over ALL windows of a stream from one staging of its frames (round 4).  mlp_mfma_kernel in window mode reads every window's
// 3 120 features through the vector cache and splits each of them into its two f16 parts again -- a frame belongs to L = 195 windows,
// so the same split is done 195 times: 57 % of the SIMD cycles of that kernel are vector instructions, 24 % matrix ones (PMC, 32 768
// streams: 7.6 ms), and every 64 rows stage the 400 KB of split weights again.  Here a workgroup owns NT <= 7 tiles of 32 consecutive
// windows of ONE stream: their frames (32 NT + L - 1) are split once into LDS, part p / k-half h / frame in 16-byte slots (a wave's 32
// rows read 32 consecutive slots: conflict-free), and window row w at k-step f (= frame f of the window: mfcc_size 16 is one
// v_mfma_f32_32x32x16_f16 step) is simply slot w + f.  The four waves split the FRAMES of the window, not the rows: wave q runs
// frames [q L/4, (q+1) L/4) for all NT tiles, so a weight fragment is fetched once per workgroup -- straight from the lane-ordered image
// (MlpDev::wwin) into registers, four frames ahead -- and used NT times; there is no barrier inside the loop (the first version staged
// weight groups through LDS for 2 tiles per wave: 39 barriers per workgroup, 52 % matrix-pipe occupancy, 4.9 ms).  The four partial
// sums of a tile meet in LDS in a fixed order ((q0 + q1) + (q2 + q3)).  Same products as kMlpF16x2 (x0 w0 + x1 w0 + x0 w1), same mean
// correction, bias, ReLU and tail layers as mlp_mfma_kernel; rows holding a frame beyond the f16 range are listed for the f32 pass.
// Shapes: mfcc_size 16, layer 1 <= 32 wide, tail layers <= 32 wide, n_win >= 32.
// BITS: the frames are staged minus the mean of the workgroup's middle window (below), so a window's logits depend on how its stream is cut
// into workgroups -- which is a function of the stream's window count alone: the same stream gives the same bits alone, in any batch and
// on every repetition (tests/test_gpu_model_pin.py), but NOT the bits of mlp_mfma_kernel, which live-stream calls with fewer than 32 new
// windows per stream take (the row's own mean): those agree within the logit gate, 2e-6 on scores.
// P3 (round 6, RP_MLP_F32): the frames are staged as THREE bf16 parts (exact) and a frame step is six v_mfma_f32_32x32x16_bf16 per tile
// (x_i w_j, i + j <= 2, smallest first) against the three-part weight image MlpDev::wwin3 -- f32-grade products, no f16 range, nothing listed;
// three planes of frames and seven accumulator tiles take two waves per SIMD.  !P3: two f16 parts (RP_MLP_F32_FAST), as described above.
// The kernel is a thin front of mlp_windows_body (rp_mlp_windows.h), which mlp_windows_bank_kernel (per-stream models) shares.

template <int NT, bool P3>
__global__ __launch_bounds__(64 * kWinWaves, P3 ? 2 : 3) void mlp_windows_kernel(
    const float *__restrict__ mfcc, size_t frame_pitch, size_t n_win, int L, unsigned blocks_per_stream, const u32x4 *__restrict__ wimg, int slots,
    int n1p, const float *__restrict__ b1, const float *__restrict__ mean, const float *__restrict__ wsum, const float *__restrict__ tail,
    int tail_floats, int n_layers, int d1, int d2, int d3, float *__restrict__ out, uint32_t *redo) {
    const size_t s = blockIdx.x / blocks_per_stream;
    const size_t w0 = (size_t)(blockIdx.x - s * blocks_per_stream) * (NT * kWinTile);
    const size_t nl = (size_t)(n_layers == 1 ? d1 : n_layers == 2 ? d2 : d3);
    const WinModel m{L, wimg, n1p, b1, wsum, tail, tail_floats, n_layers, d1, d2, d3};
    const WinWork k{mfcc + (s * frame_pitch + w0) * 16, mean + s * n_win * 16, out + s * n_win * nl, nl, w0, n_win, slots, NT,
                    redo, s * n_win, (size_t)(gridDim.x / blocks_per_stream) * n_win};
    mlp_windows_body<NT, P3>(m, k);
}

// (Written out in full, not through the helpers of rp_mlp_dev.h: see mlp_windows_sweep there.)
// The same for layer 1 wider than 32 (the Medium and Large model types: 65 / 130 outputs for 195 frames): NQ = 2 .. 5 waves, wave q owns
// the 32-output tile q for all NT row tiles and ALL frames of the window (its own slice of the weight image, four frames ahead, used NT
// times) -- no partial sums to add up; the tiles then meet in LDS row tile by row tile ([32][32 NQ + 1] floats) for the tail layers, which
// every lane of the workgroup shares (row, output phase).  mlp_mfma_kernel in window mode, which these shapes had until now: 5.6 ms
// (Medium) / 13.5 ms (Large) per 8 192 streams.
template <int NT, int NQ, bool P3>
__global__ __launch_bounds__(64 * NQ, 2) void mlp_windows_wide_kernel(
    const float *__restrict__ mfcc, size_t frame_pitch, size_t n_win, int L, unsigned blocks_per_stream, const u32x4 *__restrict__ wimg, int slots,
    int n1p, const float *__restrict__ b1, const float *__restrict__ mean, const float *__restrict__ wsum, const float *__restrict__ tail,
    int tail_floats, int n_layers, int d1, int d2, int d3, float *__restrict__ out, uint32_t *redo) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NTHR = 64 * NQ, P1 = 32 * NQ + 1;
    float *tl = reinterpret_cast<float *>(smem);                                   // tail weights
    unsigned *flag = reinterpret_cast<unsigned *>(tl + ((tail_floats + 3) & ~3));   // [slots] frame holds a value beyond the f16 range
    u32x4 *A = reinterpret_cast<u32x4 *>(flag + slots);                           // [2 parts][2 k-halves][slots]; later h1 / h2 of a row tile
    const int tid = threadIdx.x, q = tid >> 6, l = tid & 63, lr = l & 31, lh = l >> 5;
    const size_t s = blockIdx.x / blocks_per_stream;
    const size_t w0 = (size_t)(blockIdx.x - s * blocks_per_stream) * (NT * kWinTile);
    const size_t rows_here = n_win - w0 < (size_t)(NT * kWinTile) ? n_win - w0 : (size_t)(NT * kWinTile);
    const int n_real = (int)rows_here + L - 1;
    for (int i = tid; i < tail_floats; i += NTHR) tl[i] = tail[i];
    // ---- frames minus the middle window's mean -> the two f16 parts, once (as mlp_windows_kernel)
    const float *src = mfcc + (s * frame_pitch + w0) * 16;
    const float4 *cmid = reinterpret_cast<const float4 *>(mean + (s * n_win + w0 + rows_here / 2) * 16);
    {
        constexpr int MAXI = (2 * (kWinMaxTiles * kWinTile + 256) + NTHR - 1) / NTHR;
        const int h = tid & 1;
        const float4 cl = cmid[2 * h], ch = cmid[2 * h + 1];
        float4 lo[MAXI], hi[MAXI];
#pragma unroll
        for (int v = 0; v < MAXI; ++v) {
            const int i = tid + v * NTHR, fr = i >> 1;
            if (i < 2 * slots && fr < n_real) {
                lo[v] = *reinterpret_cast<const float4 *>(src + (size_t)fr * 16 + 8 * h);
                hi[v] = *reinterpret_cast<const float4 *>(src + (size_t)fr * 16 + 8 * h + 4);
            } else { lo[v] = cl; hi[v] = ch; }
        }
#pragma unroll
        for (int v = 0; v < MAXI; ++v) {
            const int i = tid + v * NTHR, fr = i >> 1;
            if (i < 2 * slots) {
                const float xs[8] = {lo[v].x - cl.x, lo[v].y - cl.y, lo[v].z - cl.z, lo[v].w - cl.w, hi[v].x - ch.x, hi[v].y - ch.y, hi[v].z - ch.z, hi[v].w - ch.w};
                u32x4 p0, p1, p2;
                float rng = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float a = xs[2 * e], b = xs[2 * e + 1];
                    if (P3) {   // a = a0 + a1 + a2 exactly: a0 = a & 0xffff0000 (a bf16), r = a - a0, a1 = r & 0xffff0000, a2 = r - a1; a packed register = two upper halves
                        const float ra = a - __uint_as_float(__float_as_uint(a) & 0xffff0000u), rb = b - __uint_as_float(__float_as_uint(b) & 0xffff0000u);
                        p0[e] = __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);
                        p1[e] = __builtin_amdgcn_perm(__float_as_uint(rb), __float_as_uint(ra), 0x07060302u);
                        p2[e] = __builtin_amdgcn_perm(__float_as_uint(rb - __uint_as_float(__float_as_uint(rb) & 0xffff0000u)),
                                                      __float_as_uint(ra - __uint_as_float(__float_as_uint(ra) & 0xffff0000u)), 0x07060302u);
                    } else {
                        rng = fmaxf(fmaxf(rng, fabsf(a)), fabsf(b));
                        p0[e] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(a, b));
                        p1[e] = pk_f16_second(a - __uint_as_float(__float_as_uint(a) & 0xffffe000u), b - __uint_as_float(__float_as_uint(b) & 0xffffe000u));
                    }
                }
                A[(0 * 2 + h) * slots + fr] = p0;
                A[(1 * 2 + h) * slots + fr] = p1;
                if (P3) A[(2 * 2 + h) * slots + fr] = p2;
                if (h == 0) flag[fr] = 0u;
                if (!(rng <= 65504.f)) flag[fr] = 1u;
            }
        }
    }
    __syncthreads();
    // ---- every frame, this wave's 32 outputs, all NT tiles
    v16f acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
    constexpr int NPART = P3 ? 3 : 2;
    u32x4 wq0[kWinAhead], wq1[kWinAhead], wq2[P3 ? kWinAhead : 1];
    auto wfetch = [&](int f, int j) __attribute__((always_inline)) {
        const int fc = f < L ? f : L - 1;
        wq0[j] = wimg[((((size_t)fc * NQ + q) * NPART + 0) * 2 + lh) * 32 + lr];
        wq1[j] = wimg[((((size_t)fc * NQ + q) * NPART + 1) * 2 + lh) * 32 + lr];
        if (P3) wq2[j] = wimg[((((size_t)fc * NQ + q) * NPART + 2) * 2 + lh) * 32 + lr];
    };
    {
#pragma unroll
        for (int j = 0; j < kWinAhead; ++j) wfetch(j, j);
        const u32x4 *A0 = A + (0 * 2 + lh) * slots + lr, *A1 = A + (1 * 2 + lh) * slots + lr;
        const u32x4 *A2 = A + ((P3 ? 2 : 0) * 2 + lh) * slots + lr;
        (void)A2;
        for (int f0 = 0; f0 < L; f0 += kWinAhead) {
#pragma unroll
            for (int j = 0; j < kWinAhead; ++j) {
                const int f = f0 + j;
                if (f < L) {   // wave-uniform
                    if (P3) {
                        const bf16x8 c0 = __builtin_bit_cast(bf16x8, wq0[j]), c1 = __builtin_bit_cast(bf16x8, wq1[j]), c2 = __builtin_bit_cast(bf16x8, wq2[j]);
                        wfetch(f + kWinAhead, j);
#pragma unroll
                        for (int t = 0; t < NT; t += 2) {
                            const bool two = t + 1 < NT;
                            const bf16x8 x0 = __builtin_bit_cast(bf16x8, A0[t * kWinTile + f]), x1 = __builtin_bit_cast(bf16x8, A1[t * kWinTile + f]),
                                         x2 = __builtin_bit_cast(bf16x8, A2[t * kWinTile + f]);
                            bf16x8 y0 = x0, y1 = x1, y2 = x2;
                            if (two) {
                                y0 = __builtin_bit_cast(bf16x8, A0[(t + 1) * kWinTile + f]); y1 = __builtin_bit_cast(bf16x8, A1[(t + 1) * kWinTile + f]);
                                y2 = __builtin_bit_cast(bf16x8, A2[(t + 1) * kWinTile + f]);
                            }
#define RP_WIN6(XA, XB, WB)                                                                                            \
                            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(XA, WB, acc[t], 0, 0, 0);                 \
                            if (two) acc[t + 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(XB, WB, acc[t + 1], 0, 0, 0);
                            RP_WIN6(x0, y0, c2) RP_WIN6(x1, y1, c1) RP_WIN6(x2, y2, c0) RP_WIN6(x0, y0, c1) RP_WIN6(x1, y1, c0) RP_WIN6(x0, y0, c0)
#undef RP_WIN6
                        }
                        continue;
                    }
                    const f16x8 b0 = __builtin_bit_cast(f16x8, wq0[j]), b1v = __builtin_bit_cast(f16x8, wq1[j]);
                    wfetch(f + kWinAhead, j);
#pragma unroll
                    for (int t = 0; t < NT; t += 2) {
                        const bool two = t + 1 < NT;
                        const f16x8 p0 = __builtin_bit_cast(f16x8, A0[t * kWinTile + f]), p1 = __builtin_bit_cast(f16x8, A1[t * kWinTile + f]);
                        f16x8 q0 = p0, q1 = p1;
                        if (two) { q0 = __builtin_bit_cast(f16x8, A0[(t + 1) * kWinTile + f]); q1 = __builtin_bit_cast(f16x8, A1[(t + 1) * kWinTile + f]); }
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(p0, b0, acc[t], 0, 0, 0);
                        if (two) acc[t + 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(q0, b0, acc[t + 1], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(p1, b0, acc[t], 0, 0, 0);
                        if (two) acc[t + 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(q1, b0, acc[t + 1], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(p0, b1v, acc[t], 0, 0, 0);
                        if (two) acc[t + 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(q0, b1v, acc[t + 1], 0, 0, 0);
                    }
                }
            }
        }
    }
    __syncthreads();   // every wave is done with the frame planes: the region becomes h1 [32][P1] and h2 [32][33] of one row tile at a time
    float *h1 = reinterpret_cast<float *>(A), *h2 = h1 + 32 * P1;
    const bool relu1 = n_layers > 1;
    const int col = 32 * q + lr;
    float4 ws4[4], c4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ws4[k] = col < n1p ? *reinterpret_cast<const float4 *>(wsum + (size_t)col * 16 + 4 * k) : make_float4(0.f, 0.f, 0.f, 0.f);
        c4[k] = cmid[k];
    }
    const float bias1 = col < n1p ? b1[col] : 0.f;
    const int prow = tid & 31, ph = tid >> 5;   // tail layers: lane = (row, output phase), 2 NQ phases
    constexpr int NPH = 2 * NQ;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const size_t wrow0 = (size_t)t * kWinTile;
        if (wrow0 >= rows_here) break;   // workgroup-uniform
        // C/D layout of the 32x32 tile: lane (column lr, half lh) holds rows 8 * (e / 4) + 4 * lh + e % 4
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = 8 * (e >> 2) + 4 * lh + (e & 3);
            size_t rr = wrow0 + row;
            if (rr >= rows_here) rr = rows_here - 1;
            const float4 *mu = reinterpret_cast<const float4 *>(mean + (s * n_win + w0 + rr) * 16);
            float corr = 0.f;   // - sum_k (mu[row][k] - c[k]) * wsum[o][k]
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 m4 = mu[k], w4 = ws4[k], c = c4[k];
                corr = fmaf(m4.x - c.x, w4.x, corr); corr = fmaf(m4.y - c.y, w4.y, corr); corr = fmaf(m4.z - c.z, w4.z, corr); corr = fmaf(m4.w - c.w, w4.w, corr);
            }
            float v = acc[t][e] - corr;
            v += bias1;
            if (relu1 && v < 0.f) v = 0.f;
            h1[row * P1 + col] = v;
        }
        __syncthreads();
        const bool row_ok = wrow0 + prow < rows_here;
        const size_t orow = s * n_win + w0 + wrow0 + prow;
        if (!P3 && ph == 0 && row_ok) {   // a window holding a frame beyond the f16 range: listed for the f32 pass
            unsigned far = 0u;
            for (int f = 0; f < L; ++f) far |= flag[wrow0 + prow + f];
            if (far) mlp_redo_append(redo, (uint32_t)orow, (size_t)(gridDim.x / blocks_per_stream) * n_win);
        }
        const int dd[4] = {d1, d2, d3, 0};
        float *dst = out + orow * (size_t)dd[n_layers - 1];
        const float *hin = h1 + prow * P1;
        if (n_layers == 1) {
            if (row_ok) for (int o = ph; o < d1; o += NPH) dst[o] = hin[o];
        } else {
            const float *wp = tl;
            int cur_in = d1;
            for (int layer = 1; layer < n_layers; ++layer) {
                const int on = dd[layer];
                const bool last = layer + 1 == n_layers;
                for (int o = ph; o < on; o += NPH) {   // sums in mlp_mfma_kernel's order
                    const float *wr = wp + (size_t)o * cur_in;
                    float s0 = 0.f, s1 = 0.f;
                    int i = 0;
                    for (; i + 1 < cur_in; i += 2) { s0 = fmaf(hin[i], wr[i], s0); s1 = fmaf(hin[i + 1], wr[i + 1], s1); }
                    if (i < cur_in) s0 = fmaf(hin[i], wr[i], s0);
                    float sacc = (s0 + s1) + wp[(size_t)on * cur_in + o];
                    if (!last && sacc < 0.f) sacc = 0.f;
                    if (last) { if (row_ok) dst[o] = sacc; } else h2[prow * 33 + o] = sacc;
                }
                __syncthreads();
                wp += (size_t)on * cur_in + on;
                cur_in = on;
                hin = h2 + prow * 33;
            }
        }
        __syncthreads();   // h1 / h2 are free for the next row tile
    }
}


// mlp_windows_kernel / mlp_windows_wide_kernel `kernel` with `waves` waves per workgroup
template <class Kernel>
static hipError_t launch_mlp_windows_kernel(Kernel kernel, int waves, hipStream_t st, const MlpDev &m, const WinRoute &r, const MlpForward &q,
                                            bool p3, uint32_t *redo) {
    if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(kernel), 160 * 1024); e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(r.bps * q.S)), dim3(64 * waves), r.lds, st, q.x, q.frame_pitch, q.n_win, m.dims[0] / 16,
                       (unsigned)r.bps, static_cast<const u32x4 *>(p3 ? m.wwin3 : m.wwin), r.slots, 16 * m.nt, m.b1, q.mean, q.wsum, m.tail,
                       m.tail_floats, m.n_layers, m.dims[1], m.dims[2], m.dims[3], q.out, redo);
    return hipGetLastError();
}

template <int NT, bool P3>
static hipError_t launch_mlp_windows_wide_nt(hipStream_t st, const MlpDev &m, const WinRoute &r, const MlpForward &q, uint32_t *redo) {
    switch (r.nq) {
    case 2: return launch_mlp_windows_kernel(mlp_windows_wide_kernel<NT, 2, P3>, 2, st, m, r, q, P3, redo);
    case 3: return launch_mlp_windows_kernel(mlp_windows_wide_kernel<NT, 3, P3>, 3, st, m, r, q, P3, redo);
    case 4: return launch_mlp_windows_kernel(mlp_windows_wide_kernel<NT, 4, P3>, 4, st, m, r, q, P3, redo);
    case 5: return launch_mlp_windows_kernel(mlp_windows_wide_kernel<NT, 5, P3>, 5, st, m, r, q, P3, redo);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_mlp_windows_wide(hipStream_t st, const MlpDev &m, const WinRoute &r, const MlpForward &q, bool p3, uint32_t *redo) {
    if (r.tiles <= 2) return p3 ? launch_mlp_windows_wide_nt<2, true>(st, m, r, q, redo) : launch_mlp_windows_wide_nt<2, false>(st, m, r, q, redo);
    return p3 ? launch_mlp_windows_wide_nt<4, true>(st, m, r, q, redo) : launch_mlp_windows_wide_nt<4, false>(st, m, r, q, redo);
}

hipError_t launch_mlp_windows(hipStream_t st, const MlpDev &m, const WinRoute &r, const MlpForward &q, bool p3, uint32_t *redo) {
    return mlp_windows_tiles(r.tiles, [&](auto nt) {
        constexpr int NT = decltype(nt)::value;
        return p3 ? launch_mlp_windows_kernel(mlp_windows_kernel<NT, true>, kWinWaves, st, m, r, q, true, redo)
                  : launch_mlp_windows_kernel(mlp_windows_kernel<NT, false>, kWinWaves, st, m, r, q, false, redo);
    });
}

// ---------------------------------------------------------------------------------------------------------------------------
// Model bank (rp_model_bank.cpp): stream s runs its OWN model bank[stream_model[s]].  mlp_windows_kernel's three-part form with the model
// read through the stream's index: a workgroup is (stream s, block b of ITS windows), cut by mlp_windows_cut from the stream's own window
// count n_frames - L(s) + 1 -- the cut rp_mlp_forward_windows gives that stream alone, hence its bits.  The grid is S x the most
// workgroups a stream of the call has, NT the most tiles a workgroup of the call owns; a workgroup behind its stream's own count leaves at
// once, tiles behind its own are skipped.  The layer-1 image (3 KB a frame of L) comes from the model's place in the bank's pool: one
// stream's workgroups share it through L2, streams of different models share nothing.  A stream with fewer than 32 windows is one partial
// tile here (the shared-model route takes mlp_mfma_kernel there: 2e-6 on scores).
template <int NT>
__global__ __launch_bounds__(64 * kWinWaves, 2) void mlp_windows_bank_kernel(ModelBankDev bank, const int32_t *__restrict__ stream_model,
                                                                             const float *__restrict__ mfcc, size_t n_frames, unsigned grid_bps,
                                                                             const float *__restrict__ mean, size_t win_pitch,
                                                                             float *__restrict__ out) {
    const size_t s = blockIdx.x / grid_bps;
    const unsigned b = blockIdx.x - (unsigned)s * grid_bps;
    const int mi = stream_model[s];
    if (mi < 0 || mi >= bank.W) return;   // no model: the row stays zero
    const ModelBankEntry e = bank.e[mi];
    if (n_frames < (size_t)e.L) return;
    const size_t n_win = n_frames - (size_t)e.L + 1;
    const WinCut cut = mlp_windows_cut(n_win);
    if (b >= cut.bps || cut.tiles > NT) return;
    const size_t w0 = (size_t)b * (size_t)(cut.tiles * kWinTile);
    const WinModel m{e.L, static_cast<const u32x4 *>(bank.wimg) + e.wimg, e.n1p, bank.b1 + e.b1, bank.wsum + e.wsum, bank.tail + e.tail,
                     e.tail_floats, e.n_layers, e.d1, e.d2, e.d3};
    const WinWork k{mfcc + (s * n_frames + w0) * 16, mean + s * win_pitch * 16, out + s * win_pitch * (size_t)bank.label_pitch,
                    (size_t)bank.label_pitch, w0, n_win, mlp_windows_slots(cut.tiles, e.L), cut.tiles, nullptr, 0, 0};
    mlp_windows_body<NT, true>(m, k);
}

void model_bank_shape_add(ModelBankShape *sh, size_t n_frames, int L, int tail_floats) {
    if (L < 1 || n_frames < (size_t)L) return;
    const WinCut cut = mlp_windows_cut(n_frames - (size_t)L + 1);
    sh->nt = std::max(sh->nt, cut.tiles);
    sh->bps = std::max(sh->bps, cut.bps);
    // three parts; sized with the largest NT of a call: the sums region grows with it
    sh->lds = std::max(sh->lds, mlp_windows_lds(tail_floats, mlp_windows_slots(cut.tiles, L), kWinMaxTiles, 3, 0));
}

hipError_t launch_mlp_windows_bank(hipStream_t st, const ModelBankDev &b, const ModelBankShape &sh, const int32_t *stream_model, const float *mfcc,
                                   size_t S, size_t n_frames, const float *mean, size_t win_pitch, float *logits) {
    if (S == 0 || win_pitch == 0 || b.label_pitch == 0) return hipSuccess;
    if (hipError_t e = hipMemsetAsync(logits, 0, S * win_pitch * (size_t)b.label_pitch * sizeof(float), st); e != hipSuccess) return e;
    if (sh.nt == 0 || sh.bps == 0) return hipSuccess;   // no stream of the call has a window
    if (S * sh.bps > 0x7fffffffULL || sh.lds > 160 * 1024) return hipErrorInvalidValue;
    return mlp_windows_tiles(sh.nt, [&](auto nt) {
        constexpr int NT = decltype(nt)::value;
        if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(mlp_windows_bank_kernel<NT>), 160 * 1024); e != hipSuccess) return e;
        hipLaunchKernelGGL(mlp_windows_bank_kernel<NT>, dim3((unsigned)(S * sh.bps)), dim3(64 * kWinWaves), sh.lds, st, b, stream_model, mfcc, n_frames,
                           sh.bps, mean, win_pitch, logits);
        return hipGetLastError();
    });
}

}  // namespace rp
