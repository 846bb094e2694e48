// The kernels of the MLSD line detector (model_mlsd.hip; the reference's MobileV2_MLSD_Large, gyre/pipeline/hinters/models/
// mbv2_mlsd_large.py) that are not planner GEMMs or convolutions.  Activations are NHWC in the storage type with 16-byte channel
// vectors per lane, arithmetic is fp32 with one rounding, every sum has a fixed order, there are no atomics and no LDS; a sample's
// result never depends on the batch it runs in.
//
//   k_mlsd_fold    BatchNorm (eval) folded into a convolution at finalize, fp32: s = gamma / sqrt(var + 1e-5), w' = w s,
//                  b' = beta + (conv_bias - mean) s; w' is rounded once to storage, b' stays fp32.  Three destination orders: a dense
//                  kxk convolution [o_pad][k k][i_pad] (the planner's), a depthwise one [9][c_pad], the entry convolution [9][4][32].
//   k_mlsd_entry   x NCHW [B][4][H][W] of a runtime dtype -> relu6(conv3x3 / stride 2 (x) + b), NHWC [B][H / 2][W / 2][32].  The
//                  reference pads one zero pixel on the right and bottom only: output o reads inputs 2 o .. 2 o + 2, zero from H (W) on.
//                  A lane owns 8 output channels of a pixel; 36 fmaf in the order tap, input channel.
//   k_mlsd_dw      depthwise 3x3 + bias + ReLU6 over [B][H][W][C]: stride 1 with zero padding 1, or stride 2 with the right / bottom
//                  padding.  A lane owns 8 channels of an output pixel; nine fmaf per channel in tap order.  relu6_in: the ReLU6 of the
//                  expand convolution in front is applied to every value read (relu6(0) = 0 keeps the padding exact), so that tensor is
//                  written once, before its activation, and never re-read for it.
//   k_mlsd_up2     bilinear x2 with align_corners=True of a C-channel map into a channel slice of a wider buffer (pixel stride ldy):
//                  source coordinate o (in - 1) / (out - 1) as the integer quotient i0 and the remainder over out - 1 (one rounding of
//                  the fraction; 0 when out == 1); relu_in: the ReLU of the 1x1 branch in front is applied on the reads.
//   k_mlsd_dconv   3x3 convolution 64 -> 64 with dilation 5 and zero padding 5, + bias + ReLU, on the 16x16x32 MFMA: a wave owns MT x 16
//                  consecutive pixels and all 64 output channels, K walks tap-major (9 taps x 2 steps of 32 channels); operand
//                  fragments are 16-byte global loads (the weights, 72 KB, stay cache resident), no LDS.
//   k_mlsd_act     in-place ReLU / ReLU6 over the first C channels of rows of pitch ld (the slice a 1x1 branch wrote into a concat)
//   k_mlsd_relu_add  y = relu(y) + x: BlockTypeB's "conv + BN + ReLU, then + x" after the planner wrote conv + bias to y
//   k_mlsd_exit    channels 7 .. 15 of the 16-channel NHWC map -> NCHW [B][9][H][W] of the output dtype
#include "kernels.h"

namespace {
// compare / select, not fminf / fmaxf: those return their other operand for a NaN, torch's relu / relu6 return the NaN
__device__ __forceinline__ float relu_f(float v) { return v <= 0.f ? 0.f : v; }
__device__ __forceinline__ float relu6_f(float v) { return v <= 0.f ? 0.f : (v >= 6.f ? 6.f : v); }
}  // namespace

// ---- BatchNorm fold ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mlsd_fold(MlsdFold a, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)a.o_pad) {                                        // the bias, by the first o_pad lanes
        float b = 0.f;
        if (i < (size_t)a.O) {
            const float s = a.gamma[i] / sqrtf(a.var[i] + 1e-5f);
            b = a.beta[i] + ((a.conv_bias ? a.conv_bias[i] : 0.f) - a.mean[i]) * s;
        }
        a.bias[i] = b;
    }
    if (i >= total) return;
    int o, src;
    bool live;
    if (a.kind == MLSD_FOLD_DENSE) {                                  // [o_pad][taps][i_pad] <- [O][I][taps]
        const int ci = (int)(i % a.i_pad);
        const size_t r = i / a.i_pad;
        const int t = (int)(r % a.taps);
        o = (int)(r / a.taps);
        live = o < a.O && ci < a.I;
        src = (o * a.I + ci) * a.taps + t;
    } else if (a.kind == MLSD_FOLD_DEPTHWISE) {                       // [9][o_pad] <- [O][1][3][3]
        o = (int)(i % a.o_pad);
        const int t = (int)(i / a.o_pad);
        live = o < a.O;
        src = o * 9 + t;
    } else {                                                          // entry: [9][I][o_pad] <- [O][I][3][3]
        o = (int)(i % a.o_pad);
        const int r = (int)(i / a.o_pad), ci = r % a.I, t = r / a.I;
        live = o < a.O;
        src = (o * a.I + ci) * 9 + t;
    }
    float v = 0.f;
    if (live) v = a.w[src] * (a.gamma[o] / sqrtf(a.var[o] + 1e-5f));
    a.out[i] = f32_to_bf16(v);
}

int launch_mlsd_fold(hipStream_t st, const MlsdFold& a) {
    if (!a.w || !a.gamma || !a.beta || !a.mean || !a.var || !a.out || !a.bias) GYRE_FAIL(-1, "mlsd_fold: null argument");
    if (a.O < 1 || a.I < 1 || a.o_pad < a.O || a.i_pad < a.I || a.kind < 0 || a.kind > 2) GYRE_FAIL(-1, "mlsd_fold: bad shape");
    if (a.kind == MLSD_FOLD_DENSE ? (a.taps != 1 && a.taps != 9) : a.taps != 9) GYRE_FAIL(-1, "mlsd_fold: 1 or 9 taps");
    const size_t total = a.kind == MLSD_FOLD_DENSE ? (size_t)a.o_pad * a.taps * a.i_pad
                       : a.kind == MLSD_FOLD_DEPTHWISE ? (size_t)9 * a.o_pad : (size_t)9 * a.I * a.o_pad;
    const size_t lanes = total > (size_t)a.o_pad ? total : (size_t)a.o_pad;
    hipLaunchKernelGGL(k_mlsd_fold, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, a, total);
    GYRE_LAUNCH_CHECK();
    return 0;
}

// ---- entry + first convolution -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mlsd_entry(const void* __restrict__ x, int dtype, int H, int W, const bf16_t* __restrict__ w,
                                                    const float* __restrict__ bias, bf16_t* __restrict__ y, size_t total) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over B * Ho * Wo * 4
    if (gid >= total) return;
    const int cg = (int)(gid & 3);
    const size_t pix = gid >> 2;
    const int Ho = H >> 1, Wo = W >> 1;
    const int ox = (int)(pix % Wo);
    const size_t t = pix / Wo;
    const int oy = (int)(t % Ho);
    const size_t b = t / Ho;
    const size_t plane = (size_t)H * W;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int iy = 2 * oy + tap / 3, ix = 2 * ox + tap % 3;
        const bool in = iy < H && ix < W;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float v = in ? load_as_f32(x, dtype, (b * 4 + c) * plane + (size_t)iy * W + ix) : 0.f;
            float wv[8];
            unpack8(*(const uint4*)(w + (tap * 4 + c) * 32 + cg * 8), wv);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = fmaf(wv[j], v, acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = relu6_f(acc[j] + bias[cg * 8 + j]);
    *(uint4*)(y + pix * 32 + cg * 8) = pack8(acc);
}

int launch_mlsd_entry(hipStream_t st, const void* x, int dtype, int B, int H, int W, const bf16_t* w, const float* bias, bf16_t* y) {
    if (!x || !w || !bias || !y) GYRE_FAIL(-1, "mlsd_entry: null argument");
    if (dtype < 0 || dtype > 2 || B < 1 || H < 2 || W < 2) GYRE_FAIL(-1, "mlsd_entry: bad dtype, or an image below 2 x 2");
    if (((size_t)w | (size_t)y) & 15) GYRE_FAIL(-6, "mlsd_entry: 16-byte alignment");
    const size_t total = (size_t)B * (H / 2) * (W / 2) * 4;
    if ((total + 255) / 256 > 0x7fffffffull) GYRE_FAIL(-1, "mlsd_entry: image too large");
    GyreProfScope prof_(KC_OTHER, st, 2.0 * 36 * 8 * total, 16.0 * total + (dtype ? 2.0 : 4.0) * 4 * B * H * W);
    hipLaunchKernelGGL(k_mlsd_entry, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, dtype, H, W, w, bias, y, total);
    GYRE_LAUNCH_CHECK();
    return 0;
}

// ---- depthwise 3x3 -------------------------------------------------------------------------------------------------------------------
template <int STRIDE, bool RELU6_IN>
__global__ __launch_bounds__(256) void k_mlsd_dw(const bf16_t* __restrict__ x, int H, int W, int C, const bf16_t* __restrict__ w,
                                                 const float* __restrict__ bias, bf16_t* __restrict__ y, size_t total) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over B * Ho * Wo * (C / 8)
    if (gid >= total) return;
    const int G = C >> 3;
    const int cg = (int)(gid % G);
    const size_t pix = gid / G;
    const int Ho = STRIDE == 2 ? H >> 1 : H, Wo = STRIDE == 2 ? W >> 1 : W;
    const int ox = (int)(pix % Wo);
    const size_t t = pix / Wo;
    const int oy = (int)(t % Ho);
    const size_t b = t / Ho;
    const int y0 = STRIDE == 2 ? 2 * oy : oy - 1, x0 = STRIDE == 2 ? 2 * ox : ox - 1;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int iy = y0 + tap / 3, ix = x0 + tap % 3;
        if ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) continue;      // zero padding: the tap adds nothing
        float v[8], wv[8];
        unpack8(*(const uint4*)(x + ((b * H + iy) * W + ix) * C + cg * 8), v);
        unpack8(*(const uint4*)(w + (size_t)tap * C + cg * 8), wv);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(wv[j], RELU6_IN ? relu6_f(v[j]) : v[j], acc[j]);
    }
    const float4 b0 = *(const float4*)(bias + cg * 8), b1 = *(const float4*)(bias + cg * 8 + 4);
    const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = relu6_f(acc[j] + bv[j]);
    *(uint4*)(y + pix * C + cg * 8) = pack8(acc);
}

int launch_mlsd_dw(hipStream_t st, const bf16_t* x, int B, int H, int W, int C, const bf16_t* w, const float* bias, int stride, int relu6_in,
                   bf16_t* y) {
    if (!x || !w || !bias || !y) GYRE_FAIL(-1, "mlsd_dw: null argument");
    if (C < 8 || C % 8) GYRE_FAIL(-6, "mlsd_dw: the channel count must be a multiple of 8");
    if (stride != 1 && stride != 2) GYRE_FAIL(-6, "mlsd_dw: stride 1 or 2");
    if (B < 1 || H < stride || W < stride) GYRE_FAIL(-1, "mlsd_dw: empty image");
    if (((size_t)x | (size_t)w | (size_t)bias | (size_t)y) & 15) GYRE_FAIL(-6, "mlsd_dw: 16-byte alignment");
    const size_t px = (size_t)B * (H / stride) * (W / stride), total = px * (C / 8);
    if ((total + 255) / 256 > 0x7fffffffull) GYRE_FAIL(-1, "mlsd_dw: image too large");
    GyreProfScope prof_(KC_OTHER, st, 18.0 * px * C, 2.0 * C * ((double)B * H * W + px));
    const dim3 grid((unsigned)((total + 255) / 256));
    if (stride == 1 && relu6_in) hipLaunchKernelGGL((k_mlsd_dw<1, true>), grid, dim3(256), 0, st, x, H, W, C, w, bias, y, total);
    else if (stride == 1) hipLaunchKernelGGL((k_mlsd_dw<1, false>), grid, dim3(256), 0, st, x, H, W, C, w, bias, y, total);
    else if (relu6_in) hipLaunchKernelGGL((k_mlsd_dw<2, true>), grid, dim3(256), 0, st, x, H, W, C, w, bias, y, total);
    else hipLaunchKernelGGL((k_mlsd_dw<2, false>), grid, dim3(256), 0, st, x, H, W, C, w, bias, y, total);
    GYRE_LAUNCH_CHECK();
    return 0;
}

// ---- bilinear x2, align_corners=True -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mlsd_up2(const bf16_t* __restrict__ x, int H, int W, int C, int ldx, int relu_in,
                                                  bf16_t* __restrict__ y, int ldy, size_t total) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over B * 2H * 2W * (C / 8)
    if (gid >= total) return;
    const int G = C >> 3;
    const int cg = (int)(gid % G);
    const size_t pix = gid / G;
    const int Ho = 2 * H, Wo = 2 * W;
    const int ox = (int)(pix % Wo);
    const size_t t = pix / Wo;
    const int oy = (int)(t % Ho);
    const size_t b = t / Ho;
    // o (in - 1) / (out - 1): quotient and remainder are exact, the fraction is rounded once (out - 1 >= 1 here: out = 2 in >= 2)
    const int ny = oy * (H - 1), nx = ox * (W - 1);
    const int i0 = ny / (Ho - 1), j0 = nx / (Wo - 1);
    const float ly = (float)(ny - i0 * (Ho - 1)) / (float)(Ho - 1), lx = (float)(nx - j0 * (Wo - 1)) / (float)(Wo - 1);
    const int i1 = i0 + (i0 < H - 1), j1 = j0 + (j0 < W - 1);
    const float wq[4] = {(1.f - ly) * (1.f - lx), (1.f - ly) * lx, ly * (1.f - lx), ly * lx};
    const int iy[4] = {i0, i0, i1, i1}, ix[4] = {j0, j1, j0, j1};
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float v[8];
        unpack8(*(const uint4*)(x + ((b * H + iy[q]) * W + ix[q]) * ldx + cg * 8), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(wq[q], relu_in ? relu_f(v[j]) : v[j], acc[j]);
    }
    *(uint4*)(y + pix * ldy + cg * 8) = pack8(acc);
}

int launch_mlsd_up2(hipStream_t st, const bf16_t* x, int B, int H, int W, int C, int ldx, int relu_in, bf16_t* y, int ldy) {
    if (!x || !y) GYRE_FAIL(-1, "mlsd_up2: null argument");
    if (C < 8 || C % 8 || ldx < C || ldy < C || ldx % 8 || ldy % 8) GYRE_FAIL(-6, "mlsd_up2: channels and pixel strides in multiples of 8");
    if (B < 1 || H < 1 || W < 1 || H > 0x3fff || W > 0x3fff) GYRE_FAIL(-1, "mlsd_up2: a map of 1 x 1 to 16383 x 16383");
    if (((size_t)x | (size_t)y) & 15) GYRE_FAIL(-6, "mlsd_up2: 16-byte alignment");
    const size_t px = (size_t)B * 4 * H * W, total = px * (C / 8);
    if ((total + 255) / 256 > 0x7fffffffull) GYRE_FAIL(-1, "mlsd_up2: image too large");
    GyreProfScope prof_(KC_OTHER, st, 8.0 * px * C, 2.0 * C * ((double)B * H * W + px));
    hipLaunchKernelGGL(k_mlsd_up2, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, H, W, C, ldx, relu_in, y, ldy, total);
    GYRE_LAUNCH_CHECK();
    return 0;
}

// ---- dilated 3x3 convolution, 64 -> 64 -----------------------------------------------------------------------------------------------
// w [64][9][64] (the planner's conv order: output channel, tap, input channel).  A wave: MT x 16 consecutive pixels of the B H W list.
// MFMA(weights, pixels): lane (fr, fq) gives rows fr (output channel of the 16-tile / pixel of the group) and k = 8 fq .. 8 fq + 7, and
// receives outputs 4 fq + e of pixel fr.
template <int MT>
__global__ __launch_bounds__(256) void k_mlsd_dconv(const bf16_t* __restrict__ x, int H, int W, const bf16_t* __restrict__ w,
                                                    const float* __restrict__ bias, bf16_t* __restrict__ y, size_t total) {
    constexpr int C = 64, DIL = 5;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const size_t base = ((size_t)blockIdx.x * 4 + wave) * (MT * 16);
    if (base >= total) return;                                         // (whole waves: no barrier follows)
    int py[MT], px[MT];
    size_t img[MT];
    bool live[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const size_t p = base + m * 16 + fr;
        live[m] = p < total;
        const size_t q = live[m] ? p : 0;
        px[m] = (int)(q % W);
        const size_t t = q / W;
        py[m] = (int)(t % H);
        img[m] = (t / H) * H * W;
    }
    f32x4_t acc[MT][4];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[m][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const bf16x8_t zero8 = __builtin_bit_cast(bf16x8_t, make_uint4(0, 0, 0, 0));
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int dy = (tap / 3 - 1) * DIL, dx = (tap % 3 - 1) * DIL;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8_t xf[MT], wf[4];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int iy = py[m] + dy, ix = px[m] + dx;
                const bool in = live[m] && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
                xf[m] = in ? *(const bf16x8_t*)(x + (img[m] + (size_t)iy * W + ix) * C + ks * 32 + fq * 8) : zero8;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[j] = *(const bf16x8_t*)(w + ((size_t)(16 * j + fr) * 9 + tap) * C + ks * 32 + fq * 8);
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[m][j] = GYRE_MFMA_16x16x32(wf[j], xf[m], acc[m][j], 0, 0, 0);
        }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        if (!live[m]) continue;
        const size_t p = base + m * 16 + fr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = 16 * j + 4 * fq;
            const float4 bv = *(const float4*)(bias + o);
            uint2 v;
            v.x = pack_bf16x2(relu_f(acc[m][j][0] + bv.x), relu_f(acc[m][j][1] + bv.y));
            v.y = pack_bf16x2(relu_f(acc[m][j][2] + bv.z), relu_f(acc[m][j][3] + bv.w));
            *(uint2*)(y + p * C + o) = v;
        }
    }
}

int launch_mlsd_dconv(hipStream_t st, const bf16_t* x, int B, int H, int W, const bf16_t* w, const float* bias, bf16_t* y) {
    if (!x || !w || !bias || !y) GYRE_FAIL(-1, "mlsd_dconv: null argument");
    if (B < 1 || H < 1 || W < 1) GYRE_FAIL(-1, "mlsd_dconv: empty image");
    if (((size_t)x | (size_t)w | (size_t)bias | (size_t)y) & 15) GYRE_FAIL(-6, "mlsd_dconv: 16-byte alignment");
    const size_t total = (size_t)B * H * W;
    constexpr int MT = 2;
    const size_t blocks = (total + 4 * MT * 16 - 1) / (4 * MT * 16);
    if (blocks > 0x7fffffffull) GYRE_FAIL(-1, "mlsd_dconv: image too large");
    GyreProfScope prof_(KC_OTHER, st, 2.0 * total * 9 * 64 * 64, 4.0 * total * 64 + 9.0 * 64 * 64 * 2);
    hipLaunchKernelGGL(k_mlsd_dconv<MT>, dim3((unsigned)blocks), dim3(256), 0, st, x, H, W, w, bias, y, total);
    GYRE_LAUNCH_CHECK();
    return 0;
}

// ---- in-place activations ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mlsd_act(bf16_t* __restrict__ x, int C, int ld, int relu6, size_t total) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over rows * (C / 8)
    if (gid >= total) return;
    const int G = C >> 3;
    bf16_t* p = x + (gid / G) * ld + (gid % G) * 8;
    float v[8];
    unpack8(*(const uint4*)p, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = relu6 ? relu6_f(v[j]) : relu_f(v[j]);
    *(uint4*)p = pack8(v);
}

int launch_mlsd_act(hipStream_t st, bf16_t* x, size_t rows, int C, int ld, int relu6) {
    if (!x) GYRE_FAIL(-1, "mlsd_act: null argument");
    if (C < 8 || C % 8 || ld < C || ld % 8 || ((size_t)x & 15)) GYRE_FAIL(-6, "mlsd_act: channels and pixel stride in multiples of 8, 16-byte alignment");
    const size_t total = rows * (C / 8);
    if (!total) return 0;
    if ((total + 255) / 256 > 0x7fffffffull) GYRE_FAIL(-1, "mlsd_act: tensor too large");
    GyreProfScope prof_(KC_OTHER, st, 1.0 * total * 8, 32.0 * total);
    hipLaunchKernelGGL(k_mlsd_act, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, C, ld, relu6, total);
    GYRE_LAUNCH_CHECK();
    return 0;
}

__global__ __launch_bounds__(256) void k_mlsd_relu_add(bf16_t* __restrict__ y, const bf16_t* __restrict__ x, size_t groups) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= groups) return;
    float a[8], b[8];
    unpack8(*(const uint4*)(y + gid * 8), a);
    unpack8(*(const uint4*)(x + gid * 8), b);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = relu_f(a[j]) + b[j];
    *(uint4*)(y + gid * 8) = pack8(a);
}

int launch_mlsd_relu_add(hipStream_t st, bf16_t* y, const bf16_t* x, size_t n) {
    if (!x || !y) GYRE_FAIL(-1, "mlsd_relu_add: null argument");
    if (n % 8 || (((size_t)x | (size_t)y) & 15)) GYRE_FAIL(-6, "mlsd_relu_add: a multiple of 8 elements, 16-byte alignment");
    if (!n) return 0;
    if ((n / 8 + 255) / 256 > 0x7fffffffull) GYRE_FAIL(-1, "mlsd_relu_add: tensor too large");
    GyreProfScope prof_(KC_OTHER, st, 2.0 * n, 6.0 * n);
    hipLaunchKernelGGL(k_mlsd_relu_add, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, st, y, x, n / 8);
    GYRE_LAUNCH_CHECK();
    return 0;
}

// ---- exit: x[:, 7:] to NCHW ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mlsd_exit(const bf16_t* __restrict__ x, size_t HW, void* __restrict__ out, int out_dtype, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;        // over B * H * W
    if (i >= total) return;
    const size_t b = i / HW, p = i - b * HW;
    float v[16];
    unpack8(*(const uint4*)(x + i * 16), v);
    unpack8(*(const uint4*)(x + i * 16 + 8), v + 8);
#pragma unroll
    for (int c = 0; c < 9; ++c) store_from_f32(out, out_dtype, (b * 9 + c) * HW + p, v[7 + c]);
}

int launch_mlsd_exit(hipStream_t st, const bf16_t* x, int B, int H, int W, void* out, int out_dtype) {
    if (!x || !out) GYRE_FAIL(-1, "mlsd_exit: null argument");
    if (B < 1 || H < 1 || W < 1 || out_dtype < 0 || out_dtype > 2) GYRE_FAIL(-1, "mlsd_exit: bad shape or dtype");
    if ((size_t)x & 15) GYRE_FAIL(-6, "mlsd_exit: 16-byte alignment");
    const size_t total = (size_t)B * H * W;
    if ((total + 255) / 256 > 0x7fffffffull) GYRE_FAIL(-1, "mlsd_exit: image too large");
    GyreProfScope prof_(KC_OTHER, st, 0.0, (32.0 + 9.0 * (out_dtype ? 2 : 4)) * total);
    hipLaunchKernelGGL(k_mlsd_exit, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, (size_t)H * W, out, out_dtype, total);
    GYRE_LAUNCH_CHECK();
    return 0;
}
