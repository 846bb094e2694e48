// UniFormer backbone kernels (model_uniformer.hip): the fused local-relation kernel of the convolutional stages, the depthwise 3x3
// position embedding every block starts with, the space-to-depth gathers in front of the patch-embedding GEMMs and the BatchNorm fold.
//
// k_uf_local<C>, C = 64 / 128 - the middle line of a CBlock, y = x + conv2(dw5x5(conv1'(x))), in ONE launch over an NHWC map
// [B][H][W] with pixel strides ldx / ldy (conv1' = conv1 with norm1 folded in, launch_uf_fold).  A workgroup of four waves owns a tile
// of UF_TH x UF_TW = 8 x 16 output pixels; with the halo of 2 that is 12 x 20 = 240 pixels = exactly 15 MFMA row tiles, so no MFMA row
// is padding.  The halo is recomputed by the neighbours: 240 / 128 = 1.875 conv1' rows per output pixel, 1.44 x the MACs of the three
// convolutions; 8 x 16 rather than 16 x 16 (1.56 rows) because the tile decides the grid - the 64 x 64 x 128 map of a 512 x 512 image is
// 32 workgroups at 8 x 16 and 16 at 16 x 16 on 256 CUs - and the LDS footprint: 77 KB at C = 128 (two workgroups per CU), 41 KB at C = 64.
// NOT MEASURED: this is reasoning from the grid and the LDS sizes.  No 16 x 16 tile was built to time against, and neither the two
// workgroups per CU at C = 128 nor what staging x in LDS (below) would cost or save has been read from a counter or a timing.
//
//   arithmetic, per pixel p and channel n (fp32 throughout, storage = the 16-bit type of the build):
//     t[p][n] = rnd(sum_k x[p][k] W1'[n][k] + b1'[n])   if p lies inside the map, else 0      one rounding.  The ZERO is the depthwise
//               convolution's padding: a halo position outside the map contributes nothing to the 5 x 5 sum - not conv1'(0) = b1'
//     d[p][n] = rnd(bd[n] + sum_{dy, dx} wd[dy][dx][n] t[p + (dy - 2, dx - 2)][n])            25 fma, (dy, dx) ascending, wd / bd fp32
//     y[p][n] = rnd(sum_k d[p][k] W2[n][k] + b2[n] + x[p][n])                                 one rounding
//   MFMA plan (v_mfma_f32_16x16x32; operand lane (fr, fq) = (lane & 15, lane >> 4) holds row / column fr and k = 8 fq .. 8 fq + 7, the
//   result lane rows 4 fq .. 4 fq + 3 of column fr).  Both products are computed TRANSPOSED, out^T = W in^T: A = weight rows, B = pixel
//   rows, so a result lane holds four consecutive channels of ONE pixel - one 8-byte store.  The channels are split over the waves:
//   wave w owns the C / 4 output channels [w C / 4, (w + 1) C / 4) of both products, C / 64 column tiles, and keeps its slices of W1'
//   and W2 as A fragments in registers for the life of the workgroup (2 x C / 64 x C / 32 fragments: 16 VGPRs at C = 64, 64 at 128);
//   the weights are read from memory once per workgroup and never per K step.
//     phase 1  per row tile m < 15: B = x[halo pixel 16 m + fr][32 ks + 8 fq ..], one 16-byte global read per K step (each of the four
//              waves reads the rows: 4 x the tile's x through L1 / L2 on top of the halo's 1.875 x.  x is not staged - staging 240 rows
//              would add 65 KB of LDS at C = 128 and leave one workgroup per CU; a deliberate, unmeasured trade);
//              + b1', the in-map select, rounding -> tile T in LDS
//     phase 2  thread = (8-channel chunk, tile column, row group): 8 / RG output rows x 8 channels of fp32 accumulators; per tap the 8
//              weights are read once from LDS (fp32 [25][C], staged transposed from the checkpoint's [C][25]) and applied to the rows;
//              16-byte LDS reads of T.  The rounded d stays in registers across a barrier and then OVERWRITES T (tile D): T is dead.
//     phase 3  per row tile m < 8 (= tile row m): B = D[16 m + fr][32 ks + 8 fq ..] from LDS; epilogue + b2 + x (8-byte global read),
//              one rounding, 8-byte global store, pixels outside the map skipped.
//   LDS: T / D [240][C + 8] storage (the pitch keeps 16-byte alignment and moves consecutive rows by 4 banks), wd [25][C] + bd [C] fp32.
//   Partial tiles: a tile position past the right / bottom edge is an out-of-map position - computed as zero, never stored.
//   y must not overlap x (a neighbour's halo reads x): refused before the launch.
//
// k_uf_cpe     - y = x + dw3x3(x) + bias, zero padding 1, NHWC, any C % 8 == 0: one thread per (pixel, 8 channels); acc = bias, nine
//                fma in (dy, dx) order on fp32 weights [9][C], + x, one rounding.  Not in place (the neighbours read x).
// k_uf_gather  - space-to-depth in front of a stride-2 patch embedding: [B][H][W][C] -> [B][H / 2][W / 2][4 C], column (2 dy + dx) C + c,
//                floor division (a trailing odd row / column is dropped as the unpadded stride-2 convolution drops it); 16-byte copies.
// k_uf_gather_img - the same for the first embedding: NCHW [B][3][H][W] of a boundary dtype -> [B][H / 4][W / 4][64], column
//                (4 ky + kx) 4 + c, rounded to storage, channel 3 of every group zero (K = 64 for the planner).
// k_uf_fold    - BatchNorm (eval) in FRONT of a 1x1 convolution folded into it, fp32, one rounding: s = gamma / sqrt(var + eps),
//                W'[o][i] = rnd(W[o][i] s[i]), b'[o] = b[o] + sum_i W[o][i] (beta[i] - mean[i] s[i]) (i ascending per lane, then the
//                lanes); exact for a 1x1 convolution fed directly by the norm.
// k_uf_taps    - depthwise weights [C][T] fp32 -> [T][C] fp32, the order the two depthwise kernels read.
#include "kernels.h"
#include "../../include/gyre_hip.h"
#include <algorithm>

namespace {
constexpr int UF_TH = 8, UF_TW = 16, UF_HH = UF_TH + 4, UF_HW = UF_TW + 4, UF_HALO = UF_HH * UF_HW;   // 240 halo pixels
static_assert(UF_HALO % 16 == 0 && UF_TW == 16, "whole MFMA row tiles; tile row m is MFMA row tile m");

struct UfLocalParams {
    const bf16_t* x; int ldx; bf16_t* y; int ldy;
    const bf16_t* w1; const float* b1;       // [C][C] storage (norm1 folded), [C]
    const float* wd; const float* bd;        // [25][C], [C] fp32
    const bf16_t* w2; const float* b2;       // [C][C] storage, [C]
    int H, W;
};

template <int C>
__global__ __launch_bounds__(256) void k_uf_local(UfLocalParams p) {
    constexpr int PITCH = C + 8, NT = C / 64, KS = C / 32, NCH = C / 8;
    constexpr int RG = 256 / (UF_TW * NCH), RY = UF_TH / RG;             // row groups of phase 2 (1 at C = 128, 2 at 64), rows per thread
    static_assert(RG >= 1 && RG * UF_TW * NCH == 256 && RY * RG == UF_TH, "phase 2 covers the tile with 256 threads");
    extern __shared__ __attribute__((aligned(16))) unsigned char uf_lds[];
    bf16_t* T = (bf16_t*)uf_lds;                                          // [240][PITCH]; rows [0, 128) become D
    float* wd = (float*)(uf_lds + (size_t)UF_HALO * PITCH * 2);           // [25][C]
    float* bd = wd + 25 * C;                                              // [C]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
    const int tx0 = blockIdx.x * UF_TW, ty0 = blockIdx.y * UF_TH;
    const size_t img = (size_t)blockIdx.z * p.H * p.W;
    const int n0 = wave * (C / 4);

    for (int i = tid; i < 26 * C; i += 256) wd[i] = i < 25 * C ? p.wd[i] : p.bd[i - 25 * C];
    bf16x8_t wf1[NT][KS], wf2[NT][KS];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const size_t o = (size_t)(n0 + 16 * j + fr) * C + 32 * ks + 8 * fq;
            wf1[j][ks] = __builtin_bit_cast(bf16x8_t, *(const uint4*)(p.w1 + o));
            wf2[j][ks] = __builtin_bit_cast(bf16x8_t, *(const uint4*)(p.w2 + o));
        }

    // ---- phase 1: T = conv1'(x) on tile + halo, zero outside the map
#pragma unroll 1
    for (int m = 0; m < UF_HALO / 16; ++m) {
        const int hp = 16 * m + fr, hy = hp / UF_HW, hx = hp - hy * UF_HW;
        const int gy = ty0 - 2 + hy, gx = tx0 - 2 + hx;
        const bool in = gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
        const bf16_t* xr = p.x + (img + (size_t)(in ? gy : 0) * p.W + (in ? gx : 0)) * p.ldx + 8 * fq;
        f32x4_t acc[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            uint4 v = {0u, 0u, 0u, 0u};
            if (in) v = *(const uint4*)(xr + 32 * ks);
            const bf16x8_t xf = __builtin_bit_cast(bf16x8_t, v);
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] = GYRE_MFMA_16x16x32(wf1[j][ks], xf, acc[j], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int n = n0 + 16 * j + 4 * fq;
            const float4 b = *(const float4*)(p.b1 + n);
            uint2 o = {0u, 0u};
            if (in) { o.x = pack_bf16x2(acc[j][0] + b.x, acc[j][1] + b.y); o.y = pack_bf16x2(acc[j][2] + b.z, acc[j][3] + b.w); }
            *(uint2*)(T + hp * PITCH + n) = o;
        }
    }
    __syncthreads();

    // ---- phase 2: d = dw5x5(T) + bd, rounded; kept in registers until every thread has finished reading T
    const int c8 = 8 * (tid % NCH), px = (tid / NCH) % UF_TW, py0 = (tid / (NCH * UF_TW)) * RY;
    float a[RY][8];
#pragma unroll
    for (int r = 0; r < RY; ++r)
#pragma unroll
        for (int e = 0; e < 8; ++e) a[r][e] = bd[c8 + e];
#pragma unroll 1
    for (int dy = 0; dy < 5; ++dy)                                        // (rolled: unrolled, the 200 reads of T are hoisted into 500 registers)
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) {
            float w8[8];
            *(float4*)w8 = *(const float4*)(wd + (dy * 5 + dx) * C + c8);
            *(float4*)(w8 + 4) = *(const float4*)(wd + (dy * 5 + dx) * C + c8 + 4);
#pragma unroll
            for (int r = 0; r < RY; ++r) {
                float v[8];
                unpack8(*(const uint4*)(T + ((py0 + r + dy) * UF_HW + px + dx) * PITCH + c8), v);
#pragma unroll
                for (int e = 0; e < 8; ++e) a[r][e] = fmaf(w8[e], v[e], a[r][e]);
            }
        }
    uint4 d8[RY];
#pragma unroll
    for (int r = 0; r < RY; ++r) d8[r] = pack8(a[r]);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RY; ++r) *(uint4*)(T + ((py0 + r) * UF_TW + px) * PITCH + c8) = d8[r];
    __syncthreads();

    // ---- phase 3: y = conv2(D) + b2 + x
#pragma unroll 1
    for (int m = 0; m < UF_TH; ++m) {
        f32x4_t acc[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const bf16x8_t df = __builtin_bit_cast(bf16x8_t, *(const uint4*)(T + (16 * m + fr) * PITCH + 32 * ks + 8 * fq));
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] = GYRE_MFMA_16x16x32(wf2[j][ks], df, acc[j], 0, 0, 0);
        }
        const int gy = ty0 + m, gx = tx0 + fr;
        if (gy < p.H && gx < p.W) {
            const size_t pix = img + (size_t)gy * p.W + gx;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int n = n0 + 16 * j + 4 * fq;
                const float4 b = *(const float4*)(p.b2 + n);
                const uint2 xr = *(const uint2*)(p.x + pix * p.ldx + n);
                uint2 o;
                o.x = pack_bf16x2(acc[j][0] + b.x + bf16lo(xr.x), acc[j][1] + b.y + bf16hi(xr.x));
                o.y = pack_bf16x2(acc[j][2] + b.z + bf16lo(xr.y), acc[j][3] + b.w + bf16hi(xr.y));
                *(uint2*)(p.y + pix * p.ldy + n) = o;
            }
        }
    }
}

// one thread per (pixel, 8 channels); w [9][C], bias [C] fp32
__global__ __launch_bounds__(256) void k_uf_cpe(const bf16_t* __restrict__ x, int H, int W, int C, size_t items, const float* __restrict__ w,
                                               const float* __restrict__ bias, bf16_t* __restrict__ y) {
    const size_t it = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const int nch = C >> 3, c = (int)(it % nch) * 8;
    const size_t pix = it / nch;
    const int px = (int)(pix % W);
    const size_t r = pix / W;
    const int py = (int)(r % H);
    const size_t img = (r / H) * H * W;
    float a[8], ctr[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { a[e] = bias[c + e]; ctr[e] = 0.f; }
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int sy = py + dy - 1, sx = px + dx - 1;
            if (sy < 0 || sy >= H || sx < 0 || sx >= W) continue;
            float v[8];
            unpack8(*(const uint4*)(x + (img + (size_t)sy * W + sx) * C + c), v);
            const float* wt = w + (dy * 3 + dx) * C + c;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                a[e] = fmaf(wt[e], v[e], a[e]);
                if (dy == 1 && dx == 1) ctr[e] = v[e];
            }
        }
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] += ctr[e];
    *(uint4*)(y + pix * C + c) = pack8(a);
}

// one thread per 16 bytes of the output
__global__ __launch_bounds__(256) void k_uf_gather(const bf16_t* __restrict__ x, int H, int W, int Ho, int Wo, int C, size_t items,
                                                  bf16_t* __restrict__ y) {
    const size_t it = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const int nch = C >> 3, c = (int)(it % nch) * 8;
    size_t r = it / nch;
    const int q = (int)(r & 3); r >>= 2;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const size_t b = r / Ho;
    const int sy = 2 * oy + (q >> 1), sx = 2 * ox + (q & 1);              // < 2 Ho <= H, < 2 Wo <= W
    const uint4 v = *(const uint4*)(x + ((b * H + sy) * (size_t)W + sx) * C + c);
    *(uint4*)(y + (((b * Ho + oy) * (size_t)Wo + ox) * 4 + q) * C + c) = v;
}

// one thread per (output pixel, ky, kx): four elements, the fourth zero
__global__ __launch_bounds__(256) void k_uf_gather_img(const void* __restrict__ x, int dtype, int H, int W, int Ho, int Wo, size_t items,
                                                      bf16_t* __restrict__ y) {
    const size_t it = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const int k = (int)(it & 15);
    size_t r = it >> 4;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const size_t b = r / Ho;
    const int sy = 4 * oy + (k >> 2), sx = 4 * ox + (k & 3);              // < 4 Ho <= H, < 4 Wo <= W
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = load_as_f32(x, dtype, ((b * 3 + c) * H + sy) * (size_t)W + sx);
    uint2 o;
    o.x = pack_bf16x2(v[0], v[1]); o.y = pack_bf16x2(v[2], 0.f);
    *(uint2*)(y + it * 4) = o;
}

// one wave per output row
__global__ __launch_bounds__(256) void k_uf_fold(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ gamma,
                                                const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ var,
                                                float eps, int O, int I, bf16_t* __restrict__ wout, float* __restrict__ bout) {
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (o >= O) return;                                  // (whole waves: no barrier follows)
    float sum = 0.f;
    for (int i = lane; i < I; i += 64) {
        const float s = gamma[i] / sqrtf(var[i] + eps), wv = w[(size_t)o * I + i];
        wout[(size_t)o * I + i] = f32_to_bf16(wv * s);
        sum = fmaf(wv, beta[i] - mean[i] * s, sum);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0) bout[o] = (b ? b[o] : 0.f) + sum;
}

__global__ void k_uf_taps(const float* __restrict__ w, int C, int T, float* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= C * T) return;
    const int t = idx / C, c = idx - t * C;
    out[idx] = w[c * T + t];
}

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}
}  // namespace

int uf_local_check(const bf16_t* x, int ldx, const bf16_t* y, int ldy, int B, int H, int W, int C, const bf16_t* w1, const float* b1,
                   const float* wd, const float* bd, const bf16_t* w2, const float* b2) {
    if (!x || !y || !w1 || !b1 || !wd || !bd || !w2 || !b2) GYRE_FAIL(GYRE_ERR_INVALID, "uf_local: null argument");
    if (B < 1 || H < 1 || W < 1) GYRE_FAIL(GYRE_ERR_INVALID, "uf_local: empty map");
    if (C != 64 && C != 128) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "uf_local: 64 and 128 channels are built");
    if (ldx < C || ldy < C) GYRE_FAIL(GYRE_ERR_INVALID, "uf_local: pixel strides below C");
    if (ldx % 8 || ldy % 4 || ((size_t)x & 15) || ((size_t)y & 7) || ((size_t)w1 & 15) || ((size_t)w2 & 15) || ((size_t)b1 & 15) || ((size_t)b2 & 15))
        GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "uf_local: x and the weights need 16-byte aligned rows, y 8-byte aligned rows");
    if (B > 65535 || (H + UF_TH - 1) / UF_TH > 65535) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "uf_local: grid limits");
    const size_t npix = (size_t)B * H * W;
    if (ranges_overlap(x, npix * ldx * 2, y, npix * ldy * 2))
        GYRE_FAIL(GYRE_ERR_INVALID, "uf_local: y must not overlap x (the neighbouring tiles read x for their halo)");
    return 0;
}
int launch_uf_local(hipStream_t st, const bf16_t* x, int ldx, bf16_t* y, int ldy, int B, int H, int W, int C, const bf16_t* w1, const float* b1,
                    const float* wd, const float* bd, const bf16_t* w2, const float* b2) {
    int rc = uf_local_check(x, ldx, y, ldy, B, H, W, C, w1, b1, wd, bd, w2, b2);
    if (rc) return rc;
    UfLocalParams p;
    p.x = x; p.ldx = ldx; p.y = y; p.ldy = ldy; p.w1 = w1; p.b1 = b1; p.wd = wd; p.bd = bd; p.w2 = w2; p.b2 = b2; p.H = H; p.W = W;
    const dim3 grid((W + UF_TW - 1) / UF_TW, (H + UF_TH - 1) / UF_TH, B);
    const size_t lds = (size_t)UF_HALO * (C + 8) * 2 + (size_t)26 * C * 4;
    const double tiles = (double)grid.x * grid.y * B, npix = (double)B * H * W;
    GyreProfScope prof(KC_OTHER, st, tiles * 2.0 * C * C * (UF_HALO + UF_TH * UF_TW) + npix * 50.0 * C, npix * C * 6.0);
#define GYRE_UF_LOCAL(C_)                                                                                                      \
    do {                                                                                                                       \
        static std::atomic<unsigned long long> attr_done{0};                                                                   \
        if (gyre_lds_attr_needed(attr_done))                                                                                   \
            (void)hipFuncSetAttribute((const void*)k_uf_local<C_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);      \
        hipLaunchKernelGGL(k_uf_local<C_>, grid, dim3(256), lds, st, p);                                                       \
    } while (0)
    if (C == 64) GYRE_UF_LOCAL(64); else GYRE_UF_LOCAL(128);
#undef GYRE_UF_LOCAL
    GYRE_LAUNCH_CHECK();
    return 0;
}
void uf_local_tile(int* th, int* tw) { *th = UF_TH; *tw = UF_TW; }

int launch_uf_cpe(hipStream_t st, const bf16_t* x, int B, int H, int W, int C, const float* w, const float* bias, bf16_t* y) {
    if (!x || !w || !bias || !y) GYRE_FAIL(GYRE_ERR_INVALID, "uf_cpe: null argument");
    if (B < 1 || H < 1 || W < 1) GYRE_FAIL(GYRE_ERR_INVALID, "uf_cpe: empty map");
    if (C < 8 || C % 8) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "uf_cpe: C must be a multiple of 8");
    if (((size_t)x | (size_t)y) & 15) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "uf_cpe: 16-byte alignment");
    const size_t items = (size_t)B * H * W * (C / 8);
    if (ranges_overlap(x, items * 16, y, items * 16)) GYRE_FAIL(GYRE_ERR_INVALID, "uf_cpe: y must not overlap x (not an in-place kernel)");
    if ((items + 255) / 256 >= (1ull << 31)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "uf_cpe: grid limits");
    GyreProfScope prof(KC_OTHER, st, 20.0 * 8 * items, 32.0 * items);
    hipLaunchKernelGGL(k_uf_cpe, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, x, H, W, C, items, w, bias, y);
    GYRE_LAUNCH_CHECK();
    return 0;
}
int launch_uf_gather(hipStream_t st, const bf16_t* x, int B, int H, int W, int C, bf16_t* y) {
    if (!x || !y) GYRE_FAIL(GYRE_ERR_INVALID, "uf_gather: null argument");
    if (B < 1 || H < 2 || W < 2) GYRE_FAIL(GYRE_ERR_INVALID, "uf_gather: a map of at least 2 x 2");
    if (C < 8 || C % 8) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "uf_gather: C must be a multiple of 8");
    if (((size_t)x | (size_t)y) & 15) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "uf_gather: 16-byte alignment");
    const int Ho = H / 2, Wo = W / 2;
    const size_t items = (size_t)B * Ho * Wo * 4 * (C / 8);
    if ((items + 255) / 256 >= (1ull << 31)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "uf_gather: grid limits");
    GyreProfScope prof(KC_OTHER, st, 0.0, 32.0 * items);
    hipLaunchKernelGGL(k_uf_gather, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, x, H, W, Ho, Wo, C, items, y);
    GYRE_LAUNCH_CHECK();
    return 0;
}
int launch_uf_gather_img(hipStream_t st, const void* x, int dtype, int B, int H, int W, bf16_t* y) {
    if (!x || !y) GYRE_FAIL(GYRE_ERR_INVALID, "uf_gather_img: null argument");
    if (dtype < 0 || dtype > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    if (B < 1 || H < 4 || W < 4) GYRE_FAIL(GYRE_ERR_INVALID, "uf_gather_img: an image of at least 4 x 4");
    if ((size_t)y & 7) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "uf_gather_img: 8-byte alignment");
    const int Ho = H / 4, Wo = W / 4;
    const size_t items = (size_t)B * Ho * Wo * 16;
    if ((items + 255) / 256 >= (1ull << 31)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "uf_gather_img: grid limits");
    GyreProfScope prof(KC_OTHER, st, 0.0, 20.0 * items);
    hipLaunchKernelGGL(k_uf_gather_img, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, x, dtype, H, W, Ho, Wo, items, y);
    GYRE_LAUNCH_CHECK();
    return 0;
}
int launch_uf_fold(hipStream_t st, const float* w, const float* b, const float* gamma, const float* beta, const float* mean, const float* var,
                   float eps, int O, int I, bf16_t* wout, float* bout) {
    if (!w || !gamma || !beta || !mean || !var || !wout || !bout) GYRE_FAIL(GYRE_ERR_INVALID, "uf_fold: null argument");
    if (O < 1 || I < 1) GYRE_FAIL(GYRE_ERR_INVALID, "uf_fold: empty matrix");
    hipLaunchKernelGGL(k_uf_fold, dim3((O + 3) / 4), dim3(256), 0, st, w, b, gamma, beta, mean, var, eps, O, I, wout, bout);
    GYRE_LAUNCH_CHECK();
    return 0;
}
int launch_uf_taps(hipStream_t st, const float* w, int C, int T, float* out) {
    if (!w || !out || C < 1 || T < 1) GYRE_FAIL(GYRE_ERR_INVALID, "uf_taps: bad argument");
    hipLaunchKernelGGL(k_uf_taps, dim3((C * T + 255) / 256), dim3(256), 0, st, w, C, T, out);
    GYRE_LAUNCH_CHECK();
    return 0;
}
