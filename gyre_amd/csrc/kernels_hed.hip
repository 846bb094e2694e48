// The kernels of the HED edge detector (model_hed.hip; the reference's HED, gyre/pipeline/hinters/models/hed.py) that are not planner
// convolutions or the in-place ReLU.  All three are streaming passes: 16-byte accesses on the storage side, fp32 arithmetic, no
// atomics, no LDS; a sample's result never depends on the batch it runs in.
//
//   k_hed_entry   x NCHW [B][3][H][W] of a runtime dtype -> the NHWC 8-channel storage tensor [B][H + 68][W + 68][8]: the image inside
//                 a zero border of 34 pixels, channels 3 .. 7 zero.  conv1_1 has padding 35; with the border in the tensor the planner
//                 runs it with its ordinary padding 1.  One lane per output pixel (one 16-byte store).
//   k_hed_tail    the end of a VGG stage in one read of the stage's last convolution BEFORE its ReLU, x [B][Hs][Ws][C]:
//                   (a) pool[b][py][px][c] = relu(max over the 2x2 window at (2 py, 2 px)), MaxPool2d(2, 2, ceil_mode=True): a window
//                       on the last row / column of an odd side holds one element per axis.  max and ReLU move storage values: exact;
//                   (b) so[b][y][x] = bias + sum_c w[c] relu(x[b][y][x][c]) in fp32, the stage's 1x1 side score.
//                 A group of C / 8 lanes owns one window: every lane holds 8 channels of its four pixels (16-byte loads), writes its
//                 8 pooled channels, and carries four partial dot products - an fmaf chain over its 8 channels, then a butterfly over
//                 the group's lanes.  The order is a function of C alone.  The ReLU tensor at full resolution is never written.
//   k_hed_fuse    one lane per output pixel: so1 at its crop offset, so2 .. so5 through their bilinear transposed convolution
//                 (kernel 2 s, stride s = 2, 4, 8, 16) evaluated in place: with Y = y + offset, i0 = Y / s and u = (Y % s + 0.5) / s
//                 the two source rows are i0 (weight u) and i0 - 1 (weight 1 - u), each only where it lies inside the map; columns
//                 alike.  u is a multiple of 1 / (2 s): the weights and their products are exact.  Then the fuse logit
//                 bf + sum_k wf[k] l_k, and the six sigmoids, fp32, one rounding to the output dtype; out [6][B][1][H][W] in the order
//                 so1 .. so5, fuse.  The crop offsets come from the host (Python's round-half-even, model_hed.hip).
#include "kernels.h"

__global__ __launch_bounds__(256) void k_hed_entry(const void* __restrict__ x, int dtype, int H, int W, bf16_t* __restrict__ y, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;        // over B * (H + 68) * (W + 68)
    if (i >= total) return;
    const int Wp = W + 2 * HED_BORDER, Hp = H + 2 * HED_BORDER;
    const int ox = (int)(i % Wp);
    const size_t t = i / Wp;
    const int oy = (int)(t % Hp);
    const size_t b = t / Hp;
    const int iy = oy - HED_BORDER, ix = ox - HED_BORDER;
    float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
        const size_t plane = (size_t)H * W, src = b * 3 * plane + (size_t)iy * W + ix;
#pragma unroll
        for (int c = 0; c < 3; ++c) f[c] = load_as_f32(x, dtype, src + c * plane);
    }
    *(uint4*)(y + i * 8) = pack8(f);
}

int launch_hed_entry(hipStream_t st, const void* x, int dtype, int B, int H, int W, bf16_t* y) {
    if (!x || !y) GYRE_FAIL(-1, "hed_entry: null argument");
    if (dtype < 0 || dtype > 2 || B < 1 || H < 1 || W < 1) GYRE_FAIL(-1, "hed_entry: bad dtype or empty image");
    if ((size_t)y & 15) GYRE_FAIL(-6, "hed_entry: 16-byte alignment");
    const size_t total = (size_t)B * (H + 2 * HED_BORDER) * (W + 2 * HED_BORDER);
    if ((total + 255) / 256 > 0x7fffffffull) GYRE_FAIL(-1, "hed_entry: image too large");
    GyreProfScope prof_(KC_OTHER, st, 0.0, 16.0 * total + (dtype ? 6.0 : 12.0) * B * H * W);
    hipLaunchKernelGGL(k_hed_entry, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, dtype, H, W, y, total);
    GYRE_LAUNCH_CHECK();
    return 0;
}

// G = C / 8 lanes per window (8, 16, 32 or 64: a wave holds 64 / G windows)
template <int G>
__global__ __launch_bounds__(256) void k_hed_tail(const bf16_t* __restrict__ x, int Hs, int Ws, const float* __restrict__ w,
                                                  const float* __restrict__ bias, bf16_t* __restrict__ pool, float* __restrict__ so,
                                                  size_t windows) {
    constexpr int C = 8 * G;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int cg = (int)(gid % G);
    const size_t win = gid / G;
    const bool live = win < windows;                   // (whole groups: every lane of a wave reaches the shuffles)
    const int Hp = (Hs + 1) >> 1, Wp = (Ws + 1) >> 1;
    const int px = (int)(win % Wp);
    const size_t t = win / Wp;
    const int py = (int)(t % Hp);
    const size_t b = t / Hp;
    const int y0 = 2 * py, x0 = 2 * px;
    const bool has_y = y0 + 1 < Hs, has_x = x0 + 1 < Ws;
    float wv[8];
    {
        const float4 w0 = *(const float4*)(w + cg * 8), w1 = *(const float4*)(w + cg * 8 + 4);
        wv[0] = w0.x; wv[1] = w0.y; wv[2] = w0.z; wv[3] = w0.w; wv[4] = w1.x; wv[5] = w1.y; wv[6] = w1.z; wv[7] = w1.w;
    }
    float m[8], dot[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const bool in = live && (!(q >> 1) || has_y) && (!(q & 1) || has_x);
        if (in) {
            float v[8];
            unpack8(*(const uint4*)(x + ((b * Hs + y0 + (q >> 1)) * Ws + x0 + (q & 1)) * C + cg * 8), v);
            float d = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                // compare / select, not fmaxf: fmaxf returns its other operand for a NaN, torch's relu and max_pool2d return the NaN
                const float r = v[j] <= 0.f ? 0.f : v[j];
                d = fmaf(wv[j], r, d);
                m[j] = q ? ((r > m[j] || r != r) ? r : m[j]) : r;      // relu(max) = max(relu): pixel 0 of a window is always inside
            }
            dot[q] = d;
        } else if (q == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) m[j] = 0.f;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int s = 1; s < G; s <<= 1) dot[q] += __shfl_xor(dot[q], s, G);
    if (!live) return;
    if (pool) *(uint4*)(pool + win * C + cg * 8) = pack8(m);
    // lane q of the group stores the score of pixel q (every lane holds all four sums)
    if (cg < 4 && (!(cg >> 1) || has_y) && (!(cg & 1) || has_x)) {
        const float d = cg == 0 ? dot[0] : cg == 1 ? dot[1] : cg == 2 ? dot[2] : dot[3];
        so[(b * Hs + y0 + (cg >> 1)) * Ws + x0 + (cg & 1)] = d + bias[0];
    }
}

int hed_tail_check(const bf16_t* x, int B, int Hs, int Ws, int C, const float* w, const float* bias, const bf16_t* pool, const float* so) {
    if (!x || !w || !bias || !so) GYRE_FAIL(-1, "hed_tail: null argument");
    if (C != 64 && C != 128 && C != 256 && C != 512) GYRE_FAIL(-6, "hed_tail: 64, 128, 256 or 512 channels are built");
    if (B < 1 || Hs < 1 || Ws < 1) GYRE_FAIL(-1, "hed_tail: empty image");
    if (((size_t)x | (size_t)pool | (size_t)w) & 15) GYRE_FAIL(-6, "hed_tail: 16-byte alignment");
    const size_t windows = (size_t)B * ((Hs + 1) / 2) * ((Ws + 1) / 2);
    if ((windows * (C / 8) + 255) / 256 > 0x7fffffffull) GYRE_FAIL(-1, "hed_tail: image too large");
    return 0;
}

int launch_hed_tail(hipStream_t st, const bf16_t* x, int B, int Hs, int Ws, int C, const float* w, const float* bias, bf16_t* pool, float* so) {
    int rc = hed_tail_check(x, B, Hs, Ws, C, w, bias, pool, so);
    if (rc) return rc;
    const size_t windows = (size_t)B * ((Hs + 1) / 2) * ((Ws + 1) / 2), px = (size_t)B * Hs * Ws;
    const dim3 grid((unsigned)((windows * (C / 8) + 255) / 256));
    GyreProfScope prof_(KC_OTHER, st, 3.0 * px * C, 2.0 * px * C + (pool ? 2.0 * windows * C : 0.0) + 4.0 * px);
    switch (C) {
        case 64: hipLaunchKernelGGL(k_hed_tail<8>, grid, dim3(256), 0, st, x, Hs, Ws, w, bias, pool, so, windows); break;
        case 128: hipLaunchKernelGGL(k_hed_tail<16>, grid, dim3(256), 0, st, x, Hs, Ws, w, bias, pool, so, windows); break;
        case 256: hipLaunchKernelGGL(k_hed_tail<32>, grid, dim3(256), 0, st, x, Hs, Ws, w, bias, pool, so, windows); break;
        default: hipLaunchKernelGGL(k_hed_tail<64>, grid, dim3(256), 0, st, x, Hs, Ws, w, bias, pool, so, windows); break;
    }
    GYRE_LAUNCH_CHECK();
    return 0;
}

// the bilinear transposed convolution of side map k (0-based: stride s = 2 << (k - 1) = 1 << k) at output pixel (Y, X) of its own frame
__device__ __forceinline__ float hed_upsample_at(const float* __restrict__ so, int Hk, int Wk, int k, int Y, int X) {
    const int s = 1 << k;
    const float inv = 1.f / (float)s;
    const int i0 = Y >> k, j0 = X >> k;
    const float uy = ((float)(Y - (i0 << k)) + 0.5f) * inv, ux = ((float)(X - (j0 << k)) + 0.5f) * inv;
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int i = i0 - a;
        if (i < 0 || i >= Hk) continue;
        const float fy = a ? 1.f - uy : uy;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int j = j0 - c;
            if (j < 0 || j >= Wk) continue;
            acc = fmaf(fy * (c ? 1.f - ux : ux), so[(size_t)i * Wk + j], acc);
        }
    }
    return acc;
}

__global__ __launch_bounds__(256) void k_hed_fuse(HedFuse a, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;        // over B * H * W
    if (i >= total) return;
    const int x = (int)(i % a.W);
    const size_t t = i / a.W;
    const int y = (int)(t % a.H);
    const size_t b = t / a.H;
    float l[5];
    l[0] = a.so[0][(b * a.Hk[0] + y + a.oy[0]) * a.Wk[0] + x + a.ox[0]];
#pragma unroll
    for (int k = 1; k < 5; ++k)
        l[k] = hed_upsample_at(a.so[k] + b * a.Hk[k] * a.Wk[k], a.Hk[k], a.Wk[k], k, y + a.oy[k], x + a.ox[k]);
    float f = a.bf[0];
#pragma unroll
    for (int k = 0; k < 5; ++k) f = fmaf(a.wf[k], l[k], f);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float v = k < 5 ? l[k] : f;
        store_from_f32(a.out, a.out_dtype, (size_t)k * total + i, 1.f / (1.f + expf(-v)));
    }
}

int hed_fuse_check(const HedFuse& a) {
    if (!a.wf || !a.bf || !a.out) GYRE_FAIL(-1, "hed_fuse: null argument");
    if (a.B < 1 || a.H < 1 || a.W < 1 || a.out_dtype < 0 || a.out_dtype > 2) GYRE_FAIL(-1, "hed_fuse: bad shape or dtype");
    for (int k = 0; k < 5; ++k) {
        if (!a.so[k]) GYRE_FAIL(-1, "hed_fuse: null score map");
        if (a.Hk[k] < 1 || a.Wk[k] < 1 || a.oy[k] < 0 || a.ox[k] < 0) GYRE_FAIL(-1, "hed_fuse: bad map size or crop offset");
        // the crop window lies inside the map (k = 0) or inside its upsampled image of (Hk + 1) s pixels
        const long long uh = k ? ((long long)a.Hk[k] + 1) << k : a.Hk[k], uw = k ? ((long long)a.Wk[k] + 1) << k : a.Wk[k];
        if ((long long)a.oy[k] + a.H > uh || (long long)a.ox[k] + a.W > uw) GYRE_FAIL(-1, "hed_fuse: the crop window leaves the map");
    }
    if (((size_t)a.B * a.H * a.W + 255) / 256 > 0x7fffffffull) GYRE_FAIL(-1, "hed_fuse: image too large");
    return 0;
}

int launch_hed_fuse(hipStream_t st, const HedFuse& a) {
    int rc = hed_fuse_check(a);
    if (rc) return rc;
    const size_t total = (size_t)a.B * a.H * a.W;
    GyreProfScope prof_(KC_OTHER, st, 60.0 * total, (4.0 + 6.0 * (a.out_dtype ? 2 : 4)) * total);
    hipLaunchKernelGGL(k_hed_fuse, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a, total);
    GYRE_LAUNCH_CHECK();
    return 0;
}
