// The kernels of the line-art hinter (model_lineart.hip; the reference's DrawingGenerator, gyre/pipeline/hinters/models/
// informative_drawings.py) that are not planner GEMMs: instance normalisation over NHWC, the sub-pixel weight composition of its
// transposed convolutions, and its two 7x7 convolutions.
//
// Instance normalisation (nn.InstanceNorm2d, affine-free, biased variance, eps 1e-5): statistics per (sample, channel) over the H W
// rows of an NHWC tensor, in fp32 and in a fixed order.
//   k_inorm_partial   one workgroup per (sample, 512-row chunk): every thread owns 8 channels and walks the chunk's rows at the
//                     workgroup's row pitch, the row lanes are then summed in ascending order.  The sums are SHIFTED by the sample's
//                     first row, s[c] = x[b][0][c]: S1 = sum (x - s), S2 = sum (x - s)^2 - a mean far from zero does not enter the
//                     squares, and a constant plane gives S1 = S2 = 0 exactly.
//   k_inorm_final     one workgroup per (sample, 32 channels): the chunk list in eight interleaved slices (chunk k in slice k % 8), each
//                     summed in ascending order, then the slices in order; mean = s + S1 / n, var = S2 / n - (S1 / n)^2 (clamped at
//                     0), rstd = 1 / sqrt(var + eps)  ->  stats [B][C][2].  (One thread walking all 512 chunks of a 512 x 512 plane
//                     was a chain of 512 dependent additions behind as many loads: half of the statistics time at batch 1, profiles/README.md.)
// No atomics; the chunks never straddle a sample, so a sample's statistics do not depend on the batch it runs in.
//   k_inorm_apply     y = (x - mean) * rstd in fp32, then the optional ReLU, then the optional residual, one rounding.  The kernel
//                     is written from the OUTPUT's side: thread i owns the i-th 16-byte piece of the output and finds its source
//                     pixel, so the forms below are one index rule each and no other copy of the tensor is ever made:
//                       pad p      the output is the (H + 2p) x (W + 2p) image with a mirrored border (nn.ReflectionPad2d(p)); a
//                                  border piece repeats the arithmetic of the interior piece it mirrors and carries its bits
//                       patch      the output row of pixel (y, x) holds the 2x2 patch (y + dy, x + dx) as 4 C columns, (dy, dx, c)
//                                  order, zeros past the last row / column: the A operand of a sub-pixel transposed convolution
//                       shuffled   the SOURCE is the output of such a convolution, [H/2][W/2][(a, b, C)] with pixel (2i + a, 2j + b)
//                                  at row (i, j), columns (2a + b) C + c; it is read in place
//                       residual   an image of the same logical size stored with a border of res_pad pixels
//
// Transposed convolution (k = 3, s = 2, p = 1, output_padding = 1) in sub-pixel form: out[2i + a][2j + b] reads x[i .. i+1][j .. j+1]
// only - a = 0: ky = 1 at i; a = 1: ky = 2 at i and ky = 0 at i + 1; columns alike.  k_tconv_compose moves the [Cin][Cout][3][3]
// weight into the [4 Cout][4 Cin] matrix of that form, rows (a, b, co), columns (dy, dx, ci); 7 of the 16 blocks stay zero.
//
// The 7x7 convolutions, both on v_mfma_f32_16x16x32 with the weights as the first operand and 16 pixels as the second, an 8 x 16
// output tile per workgroup whose 14 x 22 halo is staged in LDS once:
//   k_conv7_in    3 -> 64 channels.  The input is the 8-channel NHWC entry tensor, so a halo pixel is ONE 16-byte piece and an MFMA's
//                 K = 32 is four taps of 8 channels (13 steps for the 49 taps, the last three tap slots zero); the pad-3 reflection
//                 is the index rule of the halo load.  All weights ([64][49][8], 49 KB) sit in LDS; a workgroup walks up to four
//                 tiles of a tile row with them.
//   k_conv7_out   64 -> 1 channel over the pad-3 image the apply pass wrote: 49 taps x two 32-channel steps, only weight row 0 is
//                 live.  Bias and the optional sigmoid in fp32, written as an NCHW plane of the caller's dtype.
// Both sum in a fixed order (taps ascending), whatever the batch or the tile a pixel falls into.
#include "kernels.h"

namespace {
constexpr int IN_CHUNK = 512;              // rows per statistics workgroup
constexpr int C7_TH = 8, C7_TW = 16;       // output tile of the 7x7 kernels
constexpr int C7_HH = C7_TH + 6, C7_HW = C7_TW + 6;
constexpr int C7_IN_TILES = 4;             // tiles a k_conv7_in workgroup walks with its weights
constexpr int C7_PIXB = 144;               // k_conv7_out: bytes per halo pixel in LDS (64 channels + 16: bank spread)

// nn.ReflectionPad2d's index: i in [-pad, n + pad) with pad < n; clamped for the rows of a tile that hang over the image
__device__ __forceinline__ int reflect_idx(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * n - 2 - i : i;
    return min(max(i, 0), n - 1);
}
// v where `live`, zeros elsewhere - component by component: a select between two 16-byte objects would put the zero one on the stack
__device__ __forceinline__ uint4 keep_if(bool live, const uint4& v) {
    return make_uint4(live ? v.x : 0u, live ? v.y : 0u, live ? v.z : 0u, live ? v.w : 0u);
}
}  // namespace

size_t inorm_partial_floats(int B, size_t HW, int C) {
    return (size_t)B * ((HW + IN_CHUNK - 1) / IN_CHUNK) * 2 * (size_t)C;
}

__global__ __launch_bounds__(256) void k_inorm_partial(const bf16_t* __restrict__ x, int ld, size_t HW, int C, int nchunks,
                                                       float* __restrict__ partial) {
    __shared__ float sm[256 * 16];
    const int tid = threadIdx.x, tpr = C >> 3, lanes = 256 / tpr;
    const int cg = tid % tpr, r = tid / tpr;
    const int chunk = blockIdx.x, b = blockIdx.y;
    const bf16_t* xb = x + (size_t)b * HW * ld + cg * 8;
    float s[8], s1[8], s2[8];
    unpack8(*(const uint4*)xb, s);
#pragma unroll
    for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
    const size_t r0 = (size_t)chunk * IN_CHUNK, r1 = min(r0 + (size_t)IN_CHUNK, HW);
    for (size_t row = r0 + r; row < r1; row += lanes) {
        float v[8];
        unpack8(*(const uint4*)(xb + row * ld), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float d = v[j] - s[j];
            s1[j] += d;
            s2[j] = fmaf(d, d, s2[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) { sm[tid * 16 + j] = s1[j]; sm[tid * 16 + 8 + j] = s2[j]; }
    __syncthreads();
    if (r == 0) {
        for (int l = 1; l < lanes; ++l) {
            const float* o = sm + (l * tpr + cg) * 16;
#pragma unroll
            for (int j = 0; j < 8; ++j) { s1[j] += o[j]; s2[j] += o[8 + j]; }
        }
        float* p = partial + ((size_t)b * nchunks + chunk) * 2 * C + cg * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) { p[j] = s1[j]; p[C + j] = s2[j]; }
    }
}

__global__ __launch_bounds__(256) void k_inorm_final(const bf16_t* __restrict__ x, int ld, size_t HW, int C, int nchunks,
                                                     const float* __restrict__ partial, float eps, float* __restrict__ stats) {
    __shared__ float sm[2][8][32];
    const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl, b = blockIdx.y;
    float s1 = 0.f, s2 = 0.f;
    for (int k = sl; k < nchunks; k += 8) {
        const float* p = partial + ((size_t)b * nchunks + k) * 2 * C;
        s1 += p[c];
        s2 += p[C + c];
    }
    sm[0][sl][cl] = s1; sm[1][sl][cl] = s2;
    __syncthreads();
    if (sl) return;
    for (int j = 1; j < 8; ++j) { s1 += sm[0][j][cl]; s2 += sm[1][j][cl]; }
    const float n = (float)HW, md = s1 / n;
    float var = s2 / n - md * md;
    var = var < 0.f ? 0.f : var;               // (not fmaxf: an inf or NaN in the plane gives a NaN variance, which must reach rstd)
    stats[((size_t)b * C + c) * 2] = bf16_to_f32(x[(size_t)b * HW * ld + c]) + md;
    stats[((size_t)b * C + c) * 2 + 1] = 1.f / sqrtf(var + eps);
}

int launch_inorm_stats(hipStream_t st, const bf16_t* x, int ld, int B, size_t HW, int C, float eps, float* partial, float* stats) {
    if (!x || !partial || !stats) GYRE_FAIL(-1, "inorm_stats: null argument");
    if (C != 64 && C != 128 && C != 256) GYRE_FAIL(-6, "inorm_stats: 64, 128 or 256 channels are built");
    if (B < 1 || B > 65535 || HW < 1 || ld < C || ld % 8 || ((size_t)x & 15)) GYRE_FAIL(-1, "inorm_stats: bad shape, stride or alignment");
    const size_t nchunks = (HW + IN_CHUNK - 1) / IN_CHUNK;
    if (nchunks > 0x7fffffff) GYRE_FAIL(-6, "inorm_stats: image too large");
    GyreProfScope prof_(KC_GN_STATS, st, 3.0 * B * HW * C, 2.0 * B * HW * C);
    hipLaunchKernelGGL(k_inorm_partial, dim3((unsigned)nchunks, B), dim3(256), 0, st, x, ld, HW, C, (int)nchunks, partial);
    GYRE_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_inorm_final, dim3(C / 32, B), dim3(256), 0, st, x, ld, HW, C, (int)nchunks, partial, eps, stats);
    GYRE_LAUNCH_CHECK();
    return 0;
}

__global__ __launch_bounds__(256) void k_inorm_apply(InormApply a, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int tpr = a.C >> 3, p = a.pad;
    const int cg = (int)(i % tpr);
    size_t t = i / tpr;
    int q = 0;
    if (a.patch) { q = (int)(t & 3); t >>= 2; }
    const int OW = a.W + 2 * p, OH = a.H + 2 * p;
    const int ox = (int)(t % OW); t /= OW;
    const int oy = (int)(t % OH);
    const size_t b = t / OH;
    int y, xx;
    if (a.patch) {
        y = oy + (q >> 1); xx = ox + (q & 1);
        if (y >= a.H || xx >= a.W) { *(uint4*)(a.out + i * 8) = make_uint4(0, 0, 0, 0); return; }
    } else {
        y = reflect_idx(oy - p, a.H); xx = reflect_idx(ox - p, a.W);
    }
    size_t src;
    if (a.shuffled) {
        const int h2 = a.H >> 1, w2 = a.W >> 1;
        src = (((b * h2 + (y >> 1)) * w2 + (xx >> 1)) * 4 + ((y & 1) * 2 + (xx & 1))) * a.C;
    } else {
        src = ((b * a.H + y) * a.W + xx) * a.C;
    }
    float v[8];
    unpack8(*(const uint4*)(a.x + src + cg * 8), v);
    const float* ms = a.stats + (b * a.C + cg * 8) * 2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        v[j] = (v[j] - ms[2 * j]) * ms[2 * j + 1];
        if (a.relu) v[j] = v[j] <= 0.f ? 0.f : v[j];       // keeps a NaN, as torch's relu does (fmaxf would return 0)
    }
    if (a.res) {
        const int rp = a.res_pad;
        float rv[8];
        unpack8(*(const uint4*)(a.res + ((b * (a.H + 2 * rp) + y + rp) * (a.W + 2 * rp) + xx + rp) * a.C + cg * 8), rv);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += rv[j];
    }
    *(uint4*)(a.out + i * 8) = pack8(v);
}

int inorm_apply_check(const InormApply& a) {
    if (!a.x || !a.stats || !a.out) GYRE_FAIL(-1, "inorm_apply: null argument");
    if (a.C != 64 && a.C != 128 && a.C != 256) GYRE_FAIL(-6, "inorm_apply: 64, 128 or 256 channels are built");
    if (a.B < 1 || a.H < 1 || a.W < 1) GYRE_FAIL(-1, "inorm_apply: empty image");
    if (a.pad != 0 && a.pad != 1 && a.pad != 3) GYRE_FAIL(-6, "inorm_apply: reflection padding 0, 1 or 3 is built");
    if (a.pad >= a.H || a.pad >= a.W) GYRE_FAIL(-1, "inorm_apply: the reflection padding must be smaller than the image");
    if (a.patch && a.pad) GYRE_FAIL(-1, "inorm_apply: patch rows take no padding");
    if (a.shuffled && ((a.H | a.W) & 1)) GYRE_FAIL(-1, "inorm_apply: a shuffled source has even sides");
    if (a.res && (a.res_pad < 0 || a.res_pad > 3)) GYRE_FAIL(-1, "inorm_apply: residual border 0 to 3");
    if (((size_t)a.x | (size_t)a.out | (size_t)a.res) & 15) GYRE_FAIL(-6, "inorm_apply: 16-byte alignment");
    return 0;
}

int launch_inorm_apply(hipStream_t st, const InormApply& a) {
    int rc = inorm_apply_check(a);
    if (rc) return rc;
    const size_t total = (size_t)a.B * (a.H + 2 * a.pad) * (a.W + 2 * a.pad) * (a.patch ? 4 : 1) * (a.C >> 3);
    if ((total + 255) / 256 > 0x7fffffffull) GYRE_FAIL(-6, "inorm_apply: image too large");
    GyreProfScope prof_(KC_GN_APPLY, st, 2.0 * total * 8, 32.0 * total);
    hipLaunchKernelGGL(k_inorm_apply, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a, total);
    GYRE_LAUNCH_CHECK();
    return 0;
}

// ---- transposed-convolution weights in sub-pixel form -----------------------------------------------------------------------------
__global__ void k_tconv_compose(const void* __restrict__ w, int dtype, int Cin, int Cout, bf16_t* __restrict__ out, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int K = 4 * Cin;
    const int col = (int)(i % K), row = (int)(i / K);
    const int ci = col % Cin, d = col / Cin, co = row % Cout, ab = row / Cout;
    const int a = ab >> 1, b = ab & 1, dy = d >> 1, dx = d & 1;
    const int ky = a ? (dy ? 0 : 2) : (dy ? -1 : 1), kx = b ? (dx ? 0 : 2) : (dx ? -1 : 1);
    float v = 0.f;
    if (ky >= 0 && kx >= 0) v = load_as_f32(w, dtype, (((size_t)ci * Cout + co) * 3 + ky) * 3 + kx);
    out[i] = f32_to_bf16(v);
}

int launch_tconv_compose(hipStream_t st, const void* w, int dtype, int Cin, int Cout, bf16_t* out) {
    if (!w || !out) GYRE_FAIL(-1, "tconv_compose: null argument");
    if (dtype < 0 || dtype > 2 || Cin < 1 || Cout < 1) GYRE_FAIL(-1, "tconv_compose: bad dtype or shape");
    const size_t total = (size_t)16 * Cin * Cout;
    hipLaunchKernelGGL(k_tconv_compose, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w, dtype, Cin, Cout, out, total);
    GYRE_LAUNCH_CHECK();
    return 0;
}

// ---- first 7x7: 3 (stored as 8) -> 64 channels, reflection inside the gather --------------------------------------------------------
__global__ __launch_bounds__(256) void k_conv7_in(const bf16_t* __restrict__ x, const bf16_t* __restrict__ Wt,
                                                  const float* __restrict__ bias, bf16_t* __restrict__ out, int H, int Wd, int ntx) {
    __shared__ uint4 wl[64 * 49];                // [row][tap]: 8 channels
    __shared__ uint4 halo[C7_HH * C7_HW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int y0 = blockIdx.y * C7_TH;
    const size_t b = blockIdx.z;
    for (int i = tid; i < 64 * 49; i += 256) wl[i] = ((const uint4*)Wt)[i];
    const uint4* xb = (const uint4*)x + b * H * Wd;
    for (int t = 0; t < C7_IN_TILES; ++t) {
        const int tile = blockIdx.x * C7_IN_TILES + t;
        if (tile >= ntx) break;                  // (uniform over the workgroup)
        const int x0 = tile * C7_TW;
        __syncthreads();                         // the previous tile's fragments have been read
        for (int i = tid; i < C7_HH * C7_HW; i += 256) {
            const int py = i / C7_HW, px = i - py * C7_HW;
            halo[i] = xb[(size_t)reflect_idx(y0 - 3 + py, H) * Wd + reflect_idx(x0 - 3 + px, Wd)];
        }
        __syncthreads();
        f32x4_t acc[2][4];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) acc[g][rb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int step = 0; step < 13; ++step) {
            const int tap = 4 * step + fq;
            const bool live = tap < 49;
            const int ky = tap / 7, kx = tap - 7 * ky;
            bf16x8_t wf[4];
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) wf[rb] = __builtin_bit_cast(bf16x8_t, keep_if(live, wl[(16 * rb + fr) * 49 + (live ? tap : 0)]));
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const bf16x8_t xf = __builtin_bit_cast(bf16x8_t, keep_if(live, halo[live ? (2 * wave + g + ky) * C7_HW + fr + kx : 0]));
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) acc[g][rb] = GYRE_MFMA_16x16x32(wf[rb], xf, acc[g][rb], 0, 0, 0);
            }
        }
        // lane (fr, fq) holds channels 16 rb + 4 fq + e of pixel fr
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int gy = y0 + 2 * wave + g, gx = x0 + fr;
            if (gy >= H || gx >= Wd) continue;
            bf16_t* o = out + ((b * H + gy) * Wd + gx) * 64;
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                const int c = 16 * rb + 4 * fq;
                uint2 v;
                v.x = pack_bf16x2(acc[g][rb][0] + bias[c], acc[g][rb][1] + bias[c + 1]);
                v.y = pack_bf16x2(acc[g][rb][2] + bias[c + 2], acc[g][rb][3] + bias[c + 3]);
                *(uint2*)(o + c) = v;
            }
        }
    }
}

int launch_conv7_in(hipStream_t st, const bf16_t* x, int B, int H, int W, const bf16_t* Wt, const float* bias, bf16_t* out) {
    if (!x || !Wt || !bias || !out) GYRE_FAIL(-1, "conv7_in: null argument");
    if (B < 1 || B > 65535 || H < 4 || W < 4) GYRE_FAIL(-1, "conv7_in: the image must be at least 4 x 4 (reflection padding 3)");
    if (((size_t)x | (size_t)Wt | (size_t)out) & 15) GYRE_FAIL(-6, "conv7_in: 16-byte alignment");
    const int ntx = (W + C7_TW - 1) / C7_TW, nty = (H + C7_TH - 1) / C7_TH;
    if (nty > 65535) GYRE_FAIL(-6, "conv7_in: image too tall");
    const double px = (double)B * H * W;
    GyreProfScope prof_(KC_OTHER, st, 2.0 * px * 147 * 64, px * (16 + 128));
    hipLaunchKernelGGL(k_conv7_in, dim3((ntx + C7_IN_TILES - 1) / C7_IN_TILES, nty, B), dim3(256), 0, st, x, Wt, bias, out, H, W, ntx);
    GYRE_LAUNCH_CHECK();
    return 0;
}

// ---- last 7x7: 64 -> 1 channel over the pad-3 image, bias and sigmoid, NCHW out ---------------------------------------------------
__global__ __launch_bounds__(256) void k_conv7_out(const bf16_t* __restrict__ xp, const bf16_t* __restrict__ Wt, const float* __restrict__ bias,
                                                   int sigmoid, void* __restrict__ out, int out_dtype, int Ho, int Wo) {
    __shared__ __attribute__((aligned(16))) char halo[C7_HH * C7_HW * C7_PIXB];
    __shared__ uint4 wl[49 * 8];                 // [tap][64 channels]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int x0 = blockIdx.x * C7_TW, y0 = blockIdx.y * C7_TH;
    const size_t b = blockIdx.z;
    const int Hp = Ho + 6, Wp = Wo + 6;
    for (int i = tid; i < 49 * 8; i += 256) wl[i] = ((const uint4*)Wt)[i];
    const uint4* xb = (const uint4*)xp + b * Hp * Wp * 8;
    for (int i = tid; i < C7_HH * C7_HW * 8; i += 256) {
        const int pix = i >> 3, pc = i & 7;
        const int py = pix / C7_HW, px = pix - py * C7_HW;
        const int gy = y0 + py, gx = x0 + px;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (gy < Hp && gx < Wp) v = xb[((size_t)gy * Wp + gx) * 8 + pc];
        *(uint4*)(halo + pix * C7_PIXB + pc * 16) = v;
    }
    __syncthreads();
    f32x4_t acc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
    for (int ky = 0; ky < 7; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
            const int tap = ky * 7 + kx;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8_t wf = __builtin_bit_cast(bf16x8_t, keep_if(fr == 0, wl[tap * 8 + ks * 4 + fq]));
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const bf16x8_t xf = *(const bf16x8_t*)(halo + ((2 * wave + g + ky) * C7_HW + fr + kx) * C7_PIXB + ks * 64 + fq * 16);
                    acc[g] = GYRE_MFMA_16x16x32(wf, xf, acc[g], 0, 0, 0);
                }
            }
        }
    }
    // lane (fr, 0) holds output channel 0 of pixel fr in element 0
    if (fq == 0) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int gy = y0 + 2 * wave + g, gx = x0 + fr;
            if (gy >= Ho || gx >= Wo) continue;
            float v = acc[g][0] + bias[0];
            if (sigmoid) v = 1.f / (1.f + expf(-v));
            store_from_f32(out, out_dtype, (b * Ho + gy) * Wo + gx, v);
        }
    }
}

int launch_conv7_out(hipStream_t st, const bf16_t* xp, int B, int Ho, int Wo, const bf16_t* Wt, const float* bias, int sigmoid,
                     void* out, int out_dtype) {
    if (!xp || !Wt || !bias || !out) GYRE_FAIL(-1, "conv7_out: null argument");
    if (B < 1 || B > 65535 || Ho < 1 || Wo < 1 || out_dtype < 0 || out_dtype > 2) GYRE_FAIL(-1, "conv7_out: bad shape or dtype");
    if (((size_t)xp | (size_t)Wt) & 15) GYRE_FAIL(-6, "conv7_out: 16-byte alignment");
    const int ntx = (Wo + C7_TW - 1) / C7_TW, nty = (Ho + C7_TH - 1) / C7_TH;
    if (nty > 65535) GYRE_FAIL(-6, "conv7_out: image too tall");
    const double px = (double)B * Ho * Wo;
    GyreProfScope prof_(KC_OTHER, st, 2.0 * px * 49 * 64, px * (128 + 4));
    hipLaunchKernelGGL(k_conv7_out, dim3(ntx, nty, B), dim3(256), 0, st, xp, Wt, bias, sigmoid, out, out_dtype, Ho, Wo);
    GYRE_LAUNCH_CHECK();
    return 0;
}
