// rp_mlp_windows.h -- the body of the staged-frame window kernels that take the model through a descriptor: mlp_windows_kernel and
// mlp_windows_bank_kernel (rp_mlp_windows.hip) and mlp_windows_model_set_kernel (rp_mlp_model_set.hip) are thin fronts of mlp_windows_body.
// What the kernel computes and why is written up in rp_mlp_windows.hip.  Device code only.
#pragma once
#include "rp_mlp_dev.h"

#include <type_traits>

namespace rp {

// What a workgroup of the window kernels works with.  The model: mlp_windows_kernel gets it as kernel arguments (every stream shares it),
// mlp_windows_bank_kernel from the descriptor of its stream's model.
struct WinModel {
    int L;
    const u32x4 *wimg;    // MlpDev::wwin3 (P3) / wwin
    int n1p;              // rows of b1 / wsum
    const float *b1, *wsum, *tail;
    int tail_floats, n_layers, d1, d2, d3;
};
// Its share of one stream: windows w0 .. of the stream's n_win, nt_here <= NT tiles of them
struct WinWork {
    const float *src;     // frame w0 of the stream
    const float *mean;    // the stream's window means [n_win][16]
    float *out;           // the stream's logit rows, out_pitch floats apart
    size_t out_pitch, w0, n_win;
    int slots, nt_here;
    uint32_t *redo;       // !P3: the list of rows for the f32 pass; a row's number is redo_row0 + its window, of redo_rows in the call
    size_t redo_row0, redo_rows;
};

// a window (row `win` of the workgroup) holding a frame beyond the f16 range: listed for the f32 pass as row `row` of `rows`
__device__ __forceinline__ void mlp_windows_list(const unsigned *flag, size_t win, int L, uint32_t *redo, size_t row, size_t rows) {
    unsigned far = 0u;
    for (int f = 0; f < L; ++f) far |= flag[win + f];
    if (far) mlp_redo_append(redo, (uint32_t)row, rows);
}

// The body of both kernels.  nt_here: the tiles this workgroup owns -- the constant NT in mlp_windows_kernel (every test on it folds away),
// the stream's own count in mlp_windows_bank_kernel, whose NT is the largest of its call: tiles behind nt_here are skipped, wave-uniformly.
template <int NT, bool P3>
__device__ __forceinline__ void mlp_windows_body(const WinModel &m, const WinWork &k) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int L = m.L, slots = k.slots, nt_here = k.nt_here, n1p = m.n1p, tail_floats = m.tail_floats, n_layers = m.n_layers;
    const float *__restrict__ b1 = m.b1, *__restrict__ wsum = m.wsum, *__restrict__ tail = m.tail, *__restrict__ mean = k.mean;
    float *tl = reinterpret_cast<float *>(smem);                                   // tail weights
    unsigned *flag = reinterpret_cast<unsigned *>(tl + ((tail_floats + 3) & ~3));   // [slots] frame holds a value beyond the f16 range
    u32x4 *A = reinterpret_cast<u32x4 *>(flag + slots);                             // [2 parts][2 k-halves][slots]; later the partial sums
    const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, lr = l & 31, lh = l >> 5;
    const size_t w0 = k.w0;                                                             // first window of this workgroup
    const size_t rows_here = k.n_win - w0 < (size_t)(nt_here * kWinTile) ? k.n_win - w0 : (size_t)(nt_here * kWinTile);
    const int n_real = (int)rows_here + L - 1;                                          // frames w0 .. w0 + n_real - 1 exist
    for (int i = tid; i < tail_floats; i += 64 * kWinWaves) tl[i] = tail[i];
    // ---- frames -> the two f16 parts, once.  The window mean is taken out after layer 1 (W.(f - mu) = W.f - sum_k mu[k] wsum[k]); MFCC
    // coefficients sit on offsets many times their spread, and summing W.f with the offsets inside costs the sum their size in f32
    // rounding.  So the frames are staged minus c = the mean of the workgroup's middle window -- every window here overlaps or
    // adjoins it, so mu - c is small -- and the correction uses mu - c: W.(f - mu) = W.(f - c) - sum_k (mu - c)[k] wsum[k].
    const float4 *cmid = reinterpret_cast<const float4 *>(mean + (w0 + rows_here / 2) * 16);
    // (the splits written out, not through mlp_split_f16x2 / mlp_split_bf16x3: through them the compiler gives mlp_windows_kernel<1, true> 97
    // registers, one more than five waves per SIMD allow -- 94 with this text)
    const float *__restrict__ src = k.src;
    {
        // a thread's items are (frame i / 2, k-half i & 1 = tid & 1) for i = tid, tid + 256, ..: every load goes out before the first split
        constexpr int MAXI = (2 * (kWinMaxTiles * kWinTile + 256) + 64 * kWinWaves - 1) / (64 * kWinWaves);
        const int h = tid & 1;
        const float4 cl = cmid[2 * h], ch = cmid[2 * h + 1];
        float4 lo[MAXI], hi[MAXI];
#pragma unroll
        for (int v = 0; v < MAXI; ++v) {
            const int i = tid + v * 64 * kWinWaves, fr = i >> 1;
            if (i < 2 * slots && fr < n_real) {
                lo[v] = *reinterpret_cast<const float4 *>(src + (size_t)fr * 16 + 8 * h);
                hi[v] = *reinterpret_cast<const float4 *>(src + (size_t)fr * 16 + 8 * h + 4);
            } else { lo[v] = cl; hi[v] = ch; }   // past the real frames: zero after the offset leaves
        }
#pragma unroll
        for (int v = 0; v < MAXI; ++v) {
            const int i = tid + v * 64 * kWinWaves, fr = i >> 1;
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
                if (h == 0) flag[fr] = 0u;   // the two halves of a frame belong to neighbouring lanes of one wave: its LDS stores keep their order
                if (!(rng <= 65504.f)) flag[fr] = 1u;
            }
        }
    }
    __syncthreads();
    // ---- this wave's quarter of the frames, all NT tiles
    const int Lq = (L + kWinWaves - 1) / kWinWaves, fb = wave * Lq, fe = fb + Lq < L ? fb + Lq : L;
    v16f acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
    mlp_windows_sweep<NT, P3, 1>(A, slots, fb, fe, m.wimg, 0, nt_here, acc);
    __syncthreads();   // every wave is done with the frame planes: the region becomes the partial sums
    // ---- ((q3 + q2) + q1) + q0 through one set of sums R[tile][e / 4][lane] (16 bytes each): a wave adds what is there to its own
    // and puts the result back; one set, and h1 of a tile in that tile's own 4 KB, keep the workgroup at 48 KB = three per CU
    f32x4 *R = reinterpret_cast<f32x4 *>(A);
    auto put = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4) if (t < nt_here) R[(t * 4 + e4) * 64 + l] = f32x4{acc[t][4 * e4], acc[t][4 * e4 + 1], acc[t][4 * e4 + 2], acc[t][4 * e4 + 3]};
    };
    auto add = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4) {
                if (t >= nt_here) continue;   // wave-uniform
                const f32x4 v = R[(t * 4 + e4) * 64 + l];
                acc[t][4 * e4] = v.x + acc[t][4 * e4]; acc[t][4 * e4 + 1] = v.y + acc[t][4 * e4 + 1];
                acc[t][4 * e4 + 2] = v.z + acc[t][4 * e4 + 2]; acc[t][4 * e4 + 3] = v.w + acc[t][4 * e4 + 3];
            }
    };
    if (wave == 3) put();
    __syncthreads();
    if (wave == 2) { add(); put(); }
    __syncthreads();
    if (wave == 1) { add(); put(); }
    __syncthreads();
    if (wave == 0) { add(); put(); }
    __syncthreads();
    // ---- bias, mean correction, ReLU, tail layers: tile t by wave t % 4.  h1 [32][32] takes the place of the tile's sums, h2 [32][32] of
    // the wave sits behind the sums; column i of row r lives at (i + r) % 32: a lane walking its own row and the 32 lanes writing one
    // row both touch 32 different banks
    float *h2 = reinterpret_cast<float *>(R + NT * 4 * 64) + wave * 32 * 32;
    const bool relu1 = n_layers > 1;
    float4 ws4[4], c4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ws4[k] = lr < n1p ? *reinterpret_cast<const float4 *>(wsum + (size_t)lr * 16 + 4 * k) : make_float4(0.f, 0.f, 0.f, 0.f);
        c4[k] = cmid[k];
    }
    const float bias1 = lr < n1p ? b1[lr] : 0.f;
    for (int t = wave; t < NT; t += kWinWaves) {
        const size_t wrow0 = (size_t)t * kWinTile;   // first row of the tile inside the workgroup
        if (wrow0 >= rows_here) break;                // wave-uniform
        float *h1 = reinterpret_cast<float *>(R + t * 4 * 64);
        f32x4 sums[4];
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) sums[e4] = R[(t * 4 + e4) * 64 + l];
        wave_lds_sync();
        // C/D layout of the 32x32 tile: lane (column lr, half lh) holds rows 8 * (e / 4) + 4 * lh + e % 4
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) {
#pragma unroll
            for (int ee = 0; ee < 4; ++ee) {
                const int row = 8 * e4 + 4 * lh + ee;
                size_t rr = wrow0 + row;
                if (rr >= rows_here) rr = rows_here - 1;
                const float4 *mu = reinterpret_cast<const float4 *>(mean + (w0 + rr) * 16);
                h1[row * 32 + ((lr + row) & 31)] = mlp_windows_layer1(sums[e4][ee], mu, c4, ws4, bias1, relu1);
            }
        }
        wave_lds_sync();
        // tail layers: lane = (row lr, output phase lh), outputs strided by 2 over the phases; sums in mlp_mfma_kernel's order
        const bool row_ok = wrow0 + lr < rows_here;
        const size_t orow = w0 + wrow0 + lr;   // the window within its stream
        if (!P3 && lh == 0 && row_ok) mlp_windows_list(flag, wrow0 + lr, L, k.redo, k.redo_row0 + orow, k.redo_rows);
        mlp_tail_layers<2>(tl, n_layers, m.d1, m.d2, m.d3, 0, h1 + lr * 32, h2 + lr * 32, lh, row_ok, k.out + orow * k.out_pitch,
                           [lr](int i) { return (i + lr) & 31; }, [] { wave_lds_sync(); });
        wave_lds_sync();
    }
}

// one build per tile count a workgroup can own, 1 .. 7 (kWinMaxTiles): f(std::integral_constant<int, tiles>)
template <class F>
static hipError_t mlp_windows_tiles(int tiles, F f) {
    switch (tiles) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
    case 5: return f(std::integral_constant<int, 5>());
    case 6: return f(std::integral_constant<int, 6>());
    case 7: return f(std::integral_constant<int, 7>());
    }
    return hipErrorInvalidValue;
}

}  // namespace rp
