// Kernels of the BAE surface-normal decoder (model_bae.hip; the reference's gyre/pipeline/hinters/baenormal/submodules/decoder.py,
// Decoder in mode='test') that are not planner GEMMs or convolutions.
//
// k_bae_refine - ONE refinement stage (out_conv_res4 / res2 / res1) in one launch:
//     fine[b][:, y, x] = [norm_normalize] (W4 relu(W3 relu(W2 relu(W1 interp([x | p])(y, x) + b1) + b2) + b3) + b4)
//   x: coarse NHWC feature map [B][Hs][Ws] of CF channels in storage (pixel stride ldx), p: the coarse prediction NCHW [B][4][Hs][Ws]
//   fp32, interp: bilinear x2 with align_corners=True, fine: NCHW [B][4][2 Hs][2 Ws] fp32.  PyTorch materialises interp([x | p]) and three
//   128-channel activations at the fine resolution; here the coarse map is read once and only the four output channels are written.
//
//   Layer 1 at the COARSE resolution.  Interpolation and the 1x1 layer are linear and the four lerp weights sum to 1, so
//   W1 interp(v) + b1 = interp(W1 v + b1).  A workgroup of four waves owns a fine tile of BR_T x BR_T = 16 x 16 pixels.  With
//   s = (in - 1) / (out - 1) < 1 / 2 the 16 fine rows of a tile read coarse rows i0 in [base, base + 8] (base = int(s * first row)) and
//   i0 + 1: a footprint of BR_F x BR_F = 10 x 10 coarse pixels, coordinates clamped to the map as PyTorch clamps i1.  Phase 1 computes
//   t = W1 [x | rnd(p)] + b1 on the 100 footprint pixels (7 MFMA column tiles of 16; 12 of 112 columns are padding) and keeps t in LDS in
//   fp32 - it is never rounded.  112 / 256 = 0.44 layer-1 columns per fine pixel instead of 1.
//     MFMA plan (v_mfma_f32_16x16x32; operand lane (fr, fq) = (lane & 15, lane >> 4) holds row / column fr and k = 8 fq .. 8 fq + 7, the
//     result lane holds rows 4 fq .. 4 fq + 3 of column fr).  Every product is computed TRANSPOSED, out^T = W in^T: A = weight rows,
//     B = pixels, so a result lane holds four consecutive channels of ONE pixel.
//     phase 1  wave w owns output channels [32 w, 32 w + 32) (two row tiles) of all 7 column tiles: 56 accumulator registers.  W1
//              [128][CF + 32] streams from memory in K steps of 32 as A fragments (one 16-byte read per row tile and step), x as B
//              fragments (one 16-byte read per column tile and step; the four waves read the same x: three of the four reads hit L1).
//              The last K step holds the prediction: lanes fq = 0 carry rnd(p[0 .. 3]) and four zeros, the others zeros; W1's columns
//              above CF + 4 are zero.
//   Phases 2 - 4, per fine pixel, chained REGISTER TO REGISTER.  Wave w owns fine rows 4 w .. 4 w + 3 of the tile: four column tiles of
//   16 pixels (a tile row), all 128 channels of every layer.
//     lerp     lane (fr, fq) of column tile r lerps channels 32 ks + 8 fq .. + 7 of pixel (4 w + r, fr) from the four corners in LDS, fp32,
//              in PyTorch's form h0 (w0 a + w1 b) + h1 (w0 c + w1 d) with its fp32 coordinates (src = s * dst, i0 = int(src),
//              l1 = src - i0, l0 = 1 - l1; in == 1 gives s = 0); ReLU; ONE rounding to storage: that IS layer 2's B fragment for step ks.
//     layer 2  acc[j][r] (8 row tiles x 4 column tiles, 128 accumulator registers) += W2 fragment (16-byte LDS read, shared by the four
//              column tiles) x B.  Epilogue + b2, ReLU, one rounding.  The result lane holds channels 16 j + 4 fq .. + 3 of pixel fr; layer 3
//              wants k = 8 fq .. 8 fq + 7 per step.  An MFMA sums over its 32 k positions in any order as long as A and B agree, so step
//              ks of layer 3 takes (acc[2 ks][r], acc[2 ks + 1][r]) as it stands and W3's columns are permuted instead: LDS column
//              32 ks + 8 fq + 4 h + e holds W3's column 32 ks + 16 h + 4 fq + e.  The permutation happens while W3 is staged into LDS
//              (8-byte units), so callers pass plain weights.  No activation ever touches LDS or memory and no barrier separates the layers.
//     layer 3  the same on W3; epilogue + b3, ReLU, kept in fp32 (not rounded).
//     layer 4  128 -> 4 in fp32 on the VALU: each lane's 32 channels against W4 (fp32, LDS), j ascending, then the four fq lanes of a
//              pixel are summed by two xor shuffles (16, 32); + b4.
//     epilogue raw, or norm_normalize: n = sqrt(x^2 + y^2 + z^2) + 1e-10, (x, y, z) / n, kappa = elu(k) + 1 + 0.01 (expm1f).  Lane
//              (fr, fq) stores channel fq of pixel fr: 64-byte runs of the NCHW planes.
//   LDS (dynamic, 131 840 B: one workgroup, i.e. one wave per SIMD, per CU): t [112][132] fp32 59 136 B (the pitch of 132 words moves
//   consecutive pixels by 4 banks), W2 and W3 [128][136] storage 34 816 B each, W4 [4][128] + b2 + b3 fp32 3 072 B.  Registers: one wave
//   per SIMD leaves the whole unified file (512) to a lane; the peak is layer 2's epilogue (128 accumulators, 64 registers of layer 3
//   fragments).  W2 / W3 stay in LDS for the life of the workgroup; register to register was chosen over an LDS exchange because it
//   needs no [256][136] activation buffer (70 KB that do not fit next to t and the weights), no barriers, and reads each weight
//   fragment once per four column tiles.  16x16x32 rather than 32x32x16: the transposed result of the 16-wide form is already the next
//   layer's 8-element operand up to a column permutation; the 32-wide form's 8 x 4 row groups are not.
//   NOT MEASURED beyond tools/bae_time.py: no 32x32x16 or LDS-route variant was built to time against.
//   out must not overlap x or p: refused (GYRE_ERR_INVALID) before the launch.
//
// k_bae_up_concat - a concat buffer [B][H][W][ldo] in storage: channels [0, C) the bilinear resize (align_corners=True, ANY target size,
//   PyTorch's fp32 coordinates and lerp form, one rounding) of an NHWC storage map [B][Hs][Ws][C] (pixel stride ldx); channels
//   [C, C + Cs) the skip map, NCHW [B][Cs][H][W] of a boundary dtype, rounded once; channels [C + Cs, ldo) zero.  C == 0 is the entry
//   pass of x_block4.  One thread per (pixel, 8 channels).
// k_bae_norm8 - the first four channels of an NHWC storage map -> norm_normalize -> NCHW [B][4][HW] fp32 (out_res8).
// k_bae_exit  - fp32 -> a boundary dtype, n elements.
#include "kernels.h"
#include "../../include/gyre_hip.h"

namespace {
constexpr int BR_T = 16, BR_F = BR_T / 2 + 2, BR_FP = BR_F * BR_F, BR_MT = (BR_FP + 15) / 16;   // fine tile, footprint 10 x 10 = 100, 7 column tiles
constexpr int BR_TP = 132, BR_WP = 136, BR_H = 128, BR_PT = BR_T / 4;                           // t / weight pitches, hidden width, column tiles per wave
constexpr size_t BR_LDS = (size_t)BR_MT * 16 * BR_TP * 4 + (size_t)2 * BR_H * BR_WP * 2 + (size_t)(4 * BR_H + 2 * BR_H) * 4;
static_assert(BR_T == 16 && BR_PT == 4 && BR_H == 128, "a tile row is an MFMA column tile; four waves of four rows");

struct BaeRefineParams {
    const bf16_t* x; int ldx; const float* p; float* out;
    const bf16_t* w1; const float* b1;       // [128][CF + 32] storage, [128]
    const bf16_t* w2; const float* b2;       // [128][128] storage, [128]
    const bf16_t* w3; const float* b3;
    const float* w4; const float* b4;        // [4][128], [4] fp32
    int Hs, Ws, CF, normalize;
    float sy, sx;                            // (in - 1) / (out - 1) in fp32, as PyTorch computes it on the host
};

__device__ __forceinline__ float relu_f(float v) { return v <= 0.f ? 0.f : v; }
// norm_normalize of one pixel's four values; returns channel c
__device__ __forceinline__ float bae_normalize(float x, float y, float z, float k, int c) {
    const float n = sqrtf(x * x + y * y + z * z) + 1e-10f;
    if (c == 3) return (k > 0.f ? k : expm1f(k)) + 1.0f + 0.01f;
    return (c == 0 ? x : c == 1 ? y : z) / n;
}

__global__ __launch_bounds__(256) void k_bae_refine(BaeRefineParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bae_lds[];
    float* t = (float*)bae_lds;                                            // [112][BR_TP]
    bf16_t* w2s = (bf16_t*)(bae_lds + (size_t)BR_MT * 16 * BR_TP * 4);     // [128][BR_WP]
    bf16_t* w3s = w2s + BR_H * BR_WP;                                      // [128][BR_WP], columns permuted (header)
    float* w4s = (float*)(w3s + BR_H * BR_WP);                             // [4][128]
    float* b2s = w4s + 4 * BR_H;
    float* b3s = b2s + BR_H;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
    const int tx0 = blockIdx.x * BR_T, ty0 = blockIdx.y * BR_T, b = blockIdx.z;
    const int Hs = p.Hs, Ws = p.Ws, Ho = 2 * Hs, Wo = 2 * Ws;
    const int by = (int)(p.sy * (float)ty0), bx = (int)(p.sx * (float)tx0);      // first coarse row / column of the footprint

    // ---- stage W2, W3 (columns permuted), W4, b2, b3
    for (int i = tid; i < BR_H * 16; i += 256) {
        const int r = i >> 4, c = (i & 15) * 8;
        *(uint4*)(w2s + r * BR_WP + c) = *(const uint4*)(p.w2 + r * BR_H + c);
    }
    for (int i = tid; i < BR_H * 32; i += 256) {
        const int r = i >> 5, g = i & 31, ks = g >> 3, h = (g >> 2) & 1, q = g & 3;          // source group 8 ks + 4 h + q (4 columns each)
        *(uint2*)(w3s + r * BR_WP + 4 * (8 * ks + 2 * q + h)) = *(const uint2*)(p.w3 + r * BR_H + 4 * g);
    }
    for (int i = tid; i < 6 * BR_H; i += 256) w4s[i] = i < 4 * BR_H ? p.w4[i] : i < 5 * BR_H ? p.b2[i - 4 * BR_H] : p.b3[i - 5 * BR_H];

    // ---- phase 1: t = W1 [x | rnd(p)] + b1 on the footprint
    {
        const int n0 = 32 * wave;
        const bf16_t* xr[BR_MT];
        size_t pofs[BR_MT];
#pragma unroll
        for (int m = 0; m < BR_MT; ++m) {
            const int hp = min(16 * m + fr, BR_FP - 1), ry = hp / BR_F, rx = hp - ry * BR_F;
            const int cy = min(by + ry, Hs - 1), cx = min(bx + rx, Ws - 1);
            xr[m] = p.x + (((size_t)b * Hs + cy) * Ws + cx) * p.ldx + 8 * fq;
            pofs[m] = ((size_t)b * 4 * Hs + cy) * Ws + cx;
        }
        const bf16_t* wr0 = p.w1 + (size_t)(n0 + fr) * (p.CF + 32) + 8 * fq;
        const bf16_t* wr1 = wr0 + (size_t)16 * (p.CF + 32);
        f32x4_t acc[2][BR_MT];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int m = 0; m < BR_MT; ++m) acc[j][m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        const int KS = p.CF >> 5;
        for (int ks = 0; ks < KS; ++ks) {
            const bf16x8_t a0 = __builtin_bit_cast(bf16x8_t, *(const uint4*)(wr0 + 32 * ks));
            const bf16x8_t a1 = __builtin_bit_cast(bf16x8_t, *(const uint4*)(wr1 + 32 * ks));
#pragma unroll
            for (int m = 0; m < BR_MT; ++m) {
                const bf16x8_t xf = __builtin_bit_cast(bf16x8_t, *(const uint4*)(xr[m] + 32 * ks));
                acc[0][m] = GYRE_MFMA_16x16x32(a0, xf, acc[0][m], 0, 0, 0);
                acc[1][m] = GYRE_MFMA_16x16x32(a1, xf, acc[1][m], 0, 0, 0);
            }
        }
        {   // the prediction's K step
            const bf16x8_t a0 = __builtin_bit_cast(bf16x8_t, *(const uint4*)(wr0 + 32 * KS));
            const bf16x8_t a1 = __builtin_bit_cast(bf16x8_t, *(const uint4*)(wr1 + 32 * KS));
            const size_t plane = (size_t)Hs * Ws;
#pragma unroll
            for (int m = 0; m < BR_MT; ++m) {
                uint4 v = {0u, 0u, 0u, 0u};
                if (fq == 0) {
                    const float* pp = p.p + pofs[m];
                    v.x = pack_bf16x2(pp[0], pp[plane]);
                    v.y = pack_bf16x2(pp[2 * plane], pp[3 * plane]);
                }
                const bf16x8_t xf = __builtin_bit_cast(bf16x8_t, v);
                acc[0][m] = GYRE_MFMA_16x16x32(a0, xf, acc[0][m], 0, 0, 0);
                acc[1][m] = GYRE_MFMA_16x16x32(a1, xf, acc[1][m], 0, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + 16 * j + 4 * fq;
            const float4 bb = *(const float4*)(p.b1 + n);
#pragma unroll
            for (int m = 0; m < BR_MT; ++m)
                *(float4*)(t + (16 * m + fr) * BR_TP + n) = make_float4(acc[j][m][0] + bb.x, acc[j][m][1] + bb.y, acc[j][m][2] + bb.z, acc[j][m][3] + bb.w);
        }
    }
    __syncthreads();

    // ---- lerp + ReLU -> layer 2's B fragments
    const int gx = tx0 + fr, gy0 = ty0 + 4 * wave;
    const float srcx = p.sx * (float)gx;
    const int ix0 = (int)srcx;
    const float lx1 = srcx - (float)ix0, lx0 = 1.f - lx1;
    const int cx0 = min(ix0 - bx, BR_F - 1), cx1 = min(cx0 + (ix0 < Ws - 1 ? 1 : 0), BR_F - 1);
    uint4 bfr[BR_PT][4];
#pragma unroll
    for (int r = 0; r < BR_PT; ++r) {
        const float srcy = p.sy * (float)(gy0 + r);
        const int iy0 = (int)srcy;
        const float ly1 = srcy - (float)iy0, ly0 = 1.f - ly1;
        const int ry0 = min(iy0 - by, BR_F - 1), ry1 = min(ry0 + (iy0 < Hs - 1 ? 1 : 0), BR_F - 1);
        const float* ta = t + (ry0 * BR_F + cx0) * BR_TP + 8 * fq;
        const float* tb = t + (ry0 * BR_F + cx1) * BR_TP + 8 * fq;
        const float* tc = t + (ry1 * BR_F + cx0) * BR_TP + 8 * fq;
        const float* td = t + (ry1 * BR_F + cx1) * BR_TP + 8 * fq;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            float v[8];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int o = 32 * ks + 4 * hf;
                const float4 a = *(const float4*)(ta + o), bq = *(const float4*)(tb + o), c = *(const float4*)(tc + o), d = *(const float4*)(td + o);
                v[4 * hf + 0] = relu_f(ly0 * (lx0 * a.x + lx1 * bq.x) + ly1 * (lx0 * c.x + lx1 * d.x));
                v[4 * hf + 1] = relu_f(ly0 * (lx0 * a.y + lx1 * bq.y) + ly1 * (lx0 * c.y + lx1 * d.y));
                v[4 * hf + 2] = relu_f(ly0 * (lx0 * a.z + lx1 * bq.z) + ly1 * (lx0 * c.z + lx1 * d.z));
                v[4 * hf + 3] = relu_f(ly0 * (lx0 * a.w + lx1 * bq.w) + ly1 * (lx0 * c.w + lx1 * d.w));
            }
            bfr[r][ks] = pack8(v);
        }
    }

    // ---- layers 2 and 3, register to register
    f32x4_t acc[8][BR_PT];
#pragma unroll
    for (int layer = 0; layer < 2; ++layer) {
        const bf16_t* ws = (layer ? w3s : w2s) + fr * BR_WP + 8 * fq;
        const float* bs = (layer ? b3s : b2s) + 4 * fq;
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int r = 0; r < BR_PT; ++r) acc[j][r] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bf16x8_t a = __builtin_bit_cast(bf16x8_t, *(const uint4*)(ws + 16 * j * BR_WP + 32 * ks));
#pragma unroll
                for (int r = 0; r < BR_PT; ++r) acc[j][r] = GYRE_MFMA_16x16x32(a, __builtin_bit_cast(bf16x8_t, bfr[r][ks]), acc[j][r], 0, 0, 0);
            }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4 bb = *(const float4*)(bs + 16 * j);
#pragma unroll
            for (int r = 0; r < BR_PT; ++r) {
                acc[j][r][0] = relu_f(acc[j][r][0] + bb.x); acc[j][r][1] = relu_f(acc[j][r][1] + bb.y);
                acc[j][r][2] = relu_f(acc[j][r][2] + bb.z); acc[j][r][3] = relu_f(acc[j][r][3] + bb.w);
            }
        }
        if (layer == 0) {
#pragma unroll
            for (int r = 0; r < BR_PT; ++r)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    uint4 v;
                    v.x = pack_bf16x2(acc[2 * ks][r][0], acc[2 * ks][r][1]); v.y = pack_bf16x2(acc[2 * ks][r][2], acc[2 * ks][r][3]);
                    v.z = pack_bf16x2(acc[2 * ks + 1][r][0], acc[2 * ks + 1][r][1]); v.w = pack_bf16x2(acc[2 * ks + 1][r][2], acc[2 * ks + 1][r][3]);
                    bfr[r][ks] = v;
                }
        }
    }

    // ---- layer 4 in fp32 and the epilogue
    float s[BR_PT][4];
#pragma unroll
    for (int r = 0; r < BR_PT; ++r)
#pragma unroll
        for (int o = 0; o < 4; ++o) s[r][o] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const float4 w = *(const float4*)(w4s + o * BR_H + 16 * j + 4 * fq);
#pragma unroll
            for (int r = 0; r < BR_PT; ++r)
                s[r][o] = fmaf(w.w, acc[j][r][3], fmaf(w.z, acc[j][r][2], fmaf(w.y, acc[j][r][1], fmaf(w.x, acc[j][r][0], s[r][o]))));
        }
    const float4 b4 = *(const float4*)p.b4;
#pragma unroll
    for (int r = 0; r < BR_PT; ++r) {
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            s[r][o] += __shfl_xor(s[r][o], 16, 64);
            s[r][o] += __shfl_xor(s[r][o], 32, 64);
        }
        const float v0 = s[r][0] + b4.x, v1 = s[r][1] + b4.y, v2 = s[r][2] + b4.z, v3 = s[r][3] + b4.w;
        const float v = p.normalize ? bae_normalize(v0, v1, v2, v3, fq) : (fq == 0 ? v0 : fq == 1 ? v1 : fq == 2 ? v2 : v3);
        const int gy = gy0 + r;
        if (gy < Ho && gx < Wo) p.out[(((size_t)b * 4 + fq) * Ho + gy) * Wo + gx] = v;
    }
}

// one thread per (output pixel, 8 channels of the pitch ldo)
__global__ __launch_bounds__(256) void k_bae_up_concat(const bf16_t* __restrict__ x, int Hs, int Ws, int C, int ldx, float sy, float sx,
                                                      const void* __restrict__ skip, int sdt, int Cs, int H, int W, size_t items,
                                                      bf16_t* __restrict__ y, int ldo) {
    const size_t it = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const int nch = ldo >> 3, c = (int)(it % nch) * 8;
    const size_t pix = it / nch;
    const int ox = (int)(pix % W);
    const size_t r = pix / W;
    const int oy = (int)(r % H);
    const size_t b = r / H;
    float v[8];
    if (c < C) {
        const float srcy = sy * (float)oy, srcx = sx * (float)ox;
        const int y0 = min((int)srcy, Hs - 1), x0 = min((int)srcx, Ws - 1);
        const int y1 = y0 + (y0 < Hs - 1 ? 1 : 0), x1 = x0 + (x0 < Ws - 1 ? 1 : 0);
        const float ly1 = srcy - (float)y0, ly0 = 1.f - ly1, lx1 = srcx - (float)x0, lx0 = 1.f - lx1;
        float a[8], bq[8], cc[8], d[8];
        unpack8(*(const uint4*)(x + ((b * Hs + y0) * Ws + x0) * ldx + c), a);
        unpack8(*(const uint4*)(x + ((b * Hs + y0) * Ws + x1) * ldx + c), bq);
        unpack8(*(const uint4*)(x + ((b * Hs + y1) * Ws + x0) * ldx + c), cc);
        unpack8(*(const uint4*)(x + ((b * Hs + y1) * Ws + x1) * ldx + c), d);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = ly0 * (lx0 * a[e] + lx1 * bq[e]) + ly1 * (lx0 * cc[e] + lx1 * d[e]);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int cs = c + e - C;
            v[e] = cs < Cs ? load_as_f32(skip, sdt, ((b * Cs + cs) * H + oy) * (size_t)W + ox) : 0.f;
        }
    }
    *(uint4*)(y + pix * ldo + c) = pack8(v);
}

// one thread per pixel
__global__ __launch_bounds__(256) void k_bae_norm8(const bf16_t* __restrict__ x, int ldx, size_t HW, size_t total, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const uint2 r = *(const uint2*)(x + i * ldx);
    const float a = bf16lo(r.x), bq = bf16hi(r.x), c = bf16lo(r.y), d = bf16hi(r.y);
    const size_t b = i / HW, q = i - b * HW;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) out[(b * 4 + ch) * HW + q] = bae_normalize(a, bq, c, d, ch);
}

__global__ __launch_bounds__(256) void k_bae_exit(const float* __restrict__ x, size_t n, void* __restrict__ out, int dtype) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) store_from_f32(out, dtype, i, x[i]);
}

bool bae_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}
// (in - 1) / (out - 1) in fp32, 0 for a one-pixel output: ATen's area_pixel_compute_scale with align_corners=True
float bae_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }
}  // namespace

void bae_refine_tile(int* th, int* tw) { *th = BR_T; *tw = BR_T; }

int launch_bae_refine(hipStream_t st, const bf16_t* x, int ldx, const float* pred, int B, int Hs, int Ws, int CF, const bf16_t* w1,
                      const float* b1, const bf16_t* w2, const float* b2, const bf16_t* w3, const float* b3, const float* w4, const float* b4,
                      int normalize, float* out) {
    if (!x || !pred || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !w4 || !b4 || !out) GYRE_FAIL(GYRE_ERR_INVALID, "bae_refine: null argument");
    if (B < 1 || Hs < 1 || Ws < 1) GYRE_FAIL(GYRE_ERR_INVALID, "bae_refine: empty map");
    if (CF < 32 || CF % 32 || CF > 8192) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "bae_refine: CF must be a multiple of 32, at most 8192");
    if (ldx < CF) GYRE_FAIL(GYRE_ERR_INVALID, "bae_refine: pixel stride below CF");
    if (ldx % 8 || (((size_t)x | (size_t)w1 | (size_t)w2 | (size_t)w3 | (size_t)b1 | (size_t)b2 | (size_t)b3 | (size_t)w4 | (size_t)b4) & 15) ||
        (((size_t)pred | (size_t)out) & 3))
        GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "bae_refine: x, the weights and the biases need 16-byte aligned rows");
    const dim3 grid((2 * Ws + BR_T - 1) / BR_T, (2 * Hs + BR_T - 1) / BR_T, B);
    if (B > 65535 || grid.y > 65535 || Hs > (1 << 22) || Ws > (1 << 22)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "bae_refine: grid limits");
    const size_t cpix = (size_t)B * Hs * Ws;
    if (bae_overlap(out, cpix * 64, x, cpix * ldx * 2) || bae_overlap(out, cpix * 64, pred, cpix * 16))
        GYRE_FAIL(GYRE_ERR_INVALID, "bae_refine: out must not overlap x or p (the neighbouring tiles read both for their footprint)");
    BaeRefineParams p;
    p.x = x; p.ldx = ldx; p.p = pred; p.out = out; p.w1 = w1; p.b1 = b1; p.w2 = w2; p.b2 = b2; p.w3 = w3; p.b3 = b3; p.w4 = w4; p.b4 = b4;
    p.Hs = Hs; p.Ws = Ws; p.CF = CF; p.normalize = normalize ? 1 : 0;
    p.sy = bae_scale(Hs, 2 * Hs); p.sx = bae_scale(Ws, 2 * Ws);
    const double tiles = (double)grid.x * grid.y * B;
    GyreProfScope prof(KC_OTHER, st, tiles * 2.0 * BR_H * (16.0 * BR_MT * (CF + 32) + 256.0 * (2 * BR_H + 4)),
                       (double)cpix * (ldx * 2.0 + 16.0 + 64.0));
    static std::atomic<unsigned long long> attr_done{0};
    if (gyre_lds_attr_needed(attr_done))
        (void)hipFuncSetAttribute((const void*)k_bae_refine, hipFuncAttributeMaxDynamicSharedMemorySize, (int)BR_LDS);
    hipLaunchKernelGGL(k_bae_refine, grid, dim3(256), BR_LDS, st, p);
    GYRE_LAUNCH_CHECK();
    return 0;
}

int launch_bae_up_concat(hipStream_t st, const bf16_t* x, int B, int Hs, int Ws, int C, int ldx, const void* skip, int skip_dtype, int Cs,
                         int H, int W, bf16_t* y, int ldo) {
    if (!y || (C > 0 && !x) || (Cs > 0 && !skip)) GYRE_FAIL(GYRE_ERR_INVALID, "bae_up_concat: null argument");
    if (B < 1 || H < 1 || W < 1 || C < 0 || Cs < 0 || C + Cs < 1 || (C > 0 && (Hs < 1 || Ws < 1))) GYRE_FAIL(GYRE_ERR_INVALID, "bae_up_concat: empty map");
    if (skip_dtype < 0 || skip_dtype > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    if (C % 8 || ldo % 8 || ldo < C + Cs || (C > 0 && (ldx % 8 || ldx < C))) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "bae_up_concat: C and the pixel strides must be multiples of 8, ldo >= C + Cs");
    if ((((size_t)x | (size_t)y) & 15)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "bae_up_concat: 16-byte alignment");
    const size_t items = (size_t)B * H * W * (ldo / 8);
    if ((items + 255) / 256 >= (1ull << 31)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "bae_up_concat: grid limits");
    if (C > 0 && bae_overlap(x, (size_t)B * Hs * Ws * ldx * 2, y, items * 16)) GYRE_FAIL(GYRE_ERR_INVALID, "bae_up_concat: y must not overlap x");
    GyreProfScope prof(KC_OTHER, st, 14.0 * 8 * items, 80.0 * items);
    hipLaunchKernelGGL(k_bae_up_concat, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, x, Hs, Ws, C, ldx, bae_scale(Hs, H),
                       bae_scale(Ws, W), skip, skip_dtype, Cs, H, W, items, y, ldo);
    GYRE_LAUNCH_CHECK();
    return 0;
}

int launch_bae_norm8(hipStream_t st, const bf16_t* x, int ldx, int B, size_t HW, float* out) {
    if (!x || !out || B < 1 || HW < 1 || ldx < 4 || ldx % 4 || ((size_t)x & 7)) GYRE_FAIL(GYRE_ERR_INVALID, "bae_norm8: bad argument");
    const size_t total = (size_t)B * HW;
    hipLaunchKernelGGL(k_bae_norm8, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, ldx, HW, total, out);
    GYRE_LAUNCH_CHECK();
    return 0;
}

int launch_bae_exit(hipStream_t st, const float* x, size_t n, void* out, int dtype) {
    if (!x || !out || n < 1 || dtype < 0 || dtype > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bae_exit: bad argument");
    hipLaunchKernelGGL(k_bae_exit, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, n, out, dtype);
    GYRE_LAUNCH_CHECK();
    return 0;
}
