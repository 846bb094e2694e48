// Kernels of the RRDBNet (ESRGAN / Real-ESRGAN) upscaler graph (model_rrdb.hip; the published BasicSR RRDBNet and the reference's
// gyre/pipeline/upscalers/models/esrgan_plus.py):
//
//   k_rdb_conv<NT>      3x3 / stride 1 / zero padding 1 implicit-GEMM convolution for the tall-M, narrow-N shape of a dense block
//                       (M = pixels, N = 32 or 64 output channels, K = 9 Cin), reading a channel PREFIX of a wider NHWC buffer and
//                       writing a channel SLICE of one, with the whole residual arithmetic of the net in its epilogue
//   k_rdb_wpack         the chunk-ordered weight copy k_rdb_conv reads
//   k_rdb_epilogue      the same epilogue applied in place to a stored convolution result (the generic path on launch_gemm)
//   k_pixel_unshuffle   NCHW of a runtime dtype -> NHWC storage in torch pixel_unshuffle(r) channel order, channels padded to 32
//
// The epilogue, fp32, in exactly this order, one rounding to storage at the end (rdb_epilogue_value; no fused multiply-adds, so a
// host emulation with separate fp32 operations reproduces k_rdb_epilogue bit for bit):
//   1. v = alpha * (acc + bias[n])
//   2. if act: v = v > 0 ? v : 0.2f * v          (a NaN fails the comparison and stays a NaN through the product)
//   3. v = v + beta1 * r1[pix][n]                  (if r1)
//   4. v = v + beta2 * r2[pix][n]                  (if r2)
//
// k_rdb_conv geometry.  One 256-thread workgroup computes a 16 x 32 pixel output tile (RDB_TH x RDB_TW) of one sample; wave w owns
// the four image rows 4w .. 4w+3, each a 32-pixel MFMA column block.  v_mfma_f32_32x32x16 with A = weights (rows = output channels)
// and B = pixels (columns): lane l holds pixel l & 31 and the accumulator registers hold four groups of four consecutive channels
// (4 (l >> 5) + 8 g .. + 3), so a lane stores / reads its residuals 8 bytes at a time.  K runs over 32-channel chunks, nine taps
// per chunk, in a fixed order; no atomics, and a sample's tiles never see another sample, so results do not depend on the batch.
// Per chunk the (TH + 2) x (TW + 2) halo window (612 pixels x 64 B) and the chunk's 9 x NT x 64 B of weights are staged in LDS;
// the next chunk's global loads are issued into registers before the MFMAs of the current one.  Both LDS images have 64-byte rows
// whose four 16-byte slots are XORed with (row >> 2) & 3, so the 32 lanes of a ds_read_b128 (consecutive rows, same slot) spread
// over all banks.  Inside a chunk a halo row fragment is read once per (k step, dx) and feeds up to three taps (dy).
#include "kernels.h"
#include "gemm_shared.h"
#include "../../include/gyre_hip.h"
#include <cmath>

#define RDB_TRY(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)

namespace {
constexpr int RDB_TH = 16, RDB_TW = 32, RDB_KC = 32;
constexpr int RDB_HW = RDB_TW + 2, RDB_HALO = (RDB_TH + 2) * RDB_HW;      // 34, 612 halo pixels
constexpr int RDB_HALO_ITEMS = RDB_HALO * 4;                               // 16-byte pieces of one halo chunk
constexpr int RDB_HALO_IT = (RDB_HALO_ITEMS + 255) / 256;                  // per thread

struct RdbEpi {
    const float* bias; float alpha; int act;
    const bf16_t* r1; int ldr1; float beta1;
    const bf16_t* r2; int ldr2; float beta2;
};
struct RdbConvParams {
    const bf16_t* x; int ldx, Cin, H, W, ups;     // H, W: SOURCE size (the output is 2H x 2W with ups)
    const bf16_t* wd;                             // [Cin / 32][9][NT][32]
    bf16_t* out; int ldo, N_live;                 // out: first element of the slice
    RdbEpi e;
};
}  // namespace

__device__ __forceinline__ float rdb_epilogue_value(float acc, float bias, float alpha, int act, bool has1, float r1, float beta1,
                                                    bool has2, float r2, float beta2) {
#pragma clang fp contract(off)
    float v = alpha * (acc + bias);
    if (act) v = v > 0.f ? v : 0.2f * v;
    if (has1) { const float t = beta1 * r1; v = v + t; }
    if (has2) { const float t = beta2 * r2; v = v + t; }
    return v;
}

template <int NT>
__global__ __launch_bounds__(256) void k_rdb_conv(RdbConvParams p) {
    constexpr int NB = NT / 32;                                    // 32-channel MFMA row blocks
    constexpr int W_ITEMS = 9 * NT * 4, W_IT = (W_ITEMS + 255) / 256;
    extern __shared__ __align__(16) char rdb_smem[];
    char* s_halo = rdb_smem;
    char* s_w = rdb_smem + RDB_HALO * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int Ho = p.ups ? 2 * p.H : p.H, Wo = p.ups ? 2 * p.W : p.W;
    const int tiles_x = (Wo + RDB_TW - 1) / RDB_TW;
    const int y0 = (int)(blockIdx.x / tiles_x) * RDB_TH, x0 = (int)(blockIdx.x % tiles_x) * RDB_TW;
    const bf16_t* xb = p.x + (size_t)blockIdx.y * p.H * p.W * p.ldx;

    // this thread's pieces of a halo chunk: element offset into the sample (-1: outside the image, a zero) and LDS byte offset
    int hsrc[RDB_HALO_IT], hdst[RDB_HALO_IT];
#pragma unroll
    for (int it = 0; it < RDB_HALO_IT; ++it) {
        const int i = tid + 256 * it;
        hsrc[it] = -1; hdst[it] = -1;
        if (i < RDB_HALO_ITEMS) {
            const int pix = i >> 2, q = i & 3, hy = pix / RDB_HW, hx = pix - hy * RDB_HW;
            const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
            hdst[it] = pix * 64 + ((q ^ ((pix >> 2) & 3)) << 4);
            if (gy >= 0 && gy < Ho && gx >= 0 && gx < Wo) {
                const int sy = p.ups ? gy >> 1 : gy, sx = p.ups ? gx >> 1 : gx;
                hsrc[it] = (sy * p.W + sx) * p.ldx + q * 8;
            }
        }
    }
    uint4 hreg[RDB_HALO_IT], wreg[W_IT];
    auto fetch = [&](int kc) {
#pragma unroll
        for (int it = 0; it < RDB_HALO_IT; ++it)
            hreg[it] = hsrc[it] >= 0 ? *(const uint4*)(xb + hsrc[it] + kc * RDB_KC) : uint4{0u, 0u, 0u, 0u};
        const uint4* wsrc = (const uint4*)(p.wd + (size_t)kc * (9 * NT * RDB_KC));
#pragma unroll
        for (int it = 0; it < W_IT; ++it) {
            const int j = tid + 256 * it;
            wreg[it] = j < W_ITEMS ? wsrc[j] : uint4{0u, 0u, 0u, 0u};
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int it = 0; it < RDB_HALO_IT; ++it)
            if (hdst[it] >= 0) *(uint4*)(s_halo + hdst[it]) = hreg[it];
#pragma unroll
        for (int it = 0; it < W_IT; ++it) {
            const int j = tid + 256 * it;
            if (j < W_ITEMS) { const int row = j >> 2, q = j & 3; *(uint4*)(s_w + row * 64 + ((q ^ ((row >> 2) & 3)) << 4)) = wreg[it]; }
        }
    };

    f32x16_t acc[4][NB];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[m][nb] = f32x16_t{};

    const int nchunks = p.Cin / RDB_KC;
    fetch(0);
    for (int kc = 0; kc < nchunks; ++kc) {
        __syncthreads();                                   // every wave has finished reading the previous chunk
        stage();
        __syncthreads();
        if (kc + 1 < nchunks) fetch(kc + 1);               // in flight under the MFMAs below
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int q = 2 * s + h;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                bf16x8_t a[3][NB];
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) {
                        const int row = (dy * 3 + dx) * NT + nb * 32 + r;
                        a[dy][nb] = *(const bf16x8_t*)(s_w + row * 64 + ((q ^ ((row >> 2) & 3)) << 4));
                    }
#pragma unroll
                for (int hr = 0; hr < 6; ++hr) {
                    const int pix = (wave * 4 + hr) * RDB_HW + r + dx;
                    const bf16x8_t bfrag = *(const bf16x8_t*)(s_halo + pix * 64 + ((q ^ ((pix >> 2) & 3)) << 4));
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy) {
                        const int m = hr - dy;
                        if (m >= 0 && m < 4) {
#pragma unroll
                            for (int nb = 0; nb < NB; ++nb) acc[m][nb] = GYRE_MFMA_32x32x16(a[dy][nb], bfrag, acc[m][nb], 0, 0, 0);
                        }
                    }
                }
            }
        }
    }

    // epilogue: lane = pixel x0 + r of row y0 + 4 wave + m; register group g = channels nb * 32 + 8 g + 4 h .. + 3
    const int gx = x0 + r;
    if (gx >= Wo) return;
    const RdbEpi& e = p.e;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int gy = y0 + wave * 4 + m;
        if (gy >= Ho) continue;
        const size_t pix = ((size_t)blockIdx.y * Ho + gy) * Wo + gx;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n0 = nb * 32 + 8 * g + 4 * h;
                if (n0 >= p.N_live) continue;
                const bool full = n0 + 4 <= p.N_live;
                float r1v[4] = {0.f, 0.f, 0.f, 0.f}, r2v[4] = {0.f, 0.f, 0.f, 0.f}, v[4];
                if (full) {
                    if (e.r1) { const uint2 t = *(const uint2*)(e.r1 + pix * e.ldr1 + n0); r1v[0] = bf16lo(t.x); r1v[1] = bf16hi(t.x); r1v[2] = bf16lo(t.y); r1v[3] = bf16hi(t.y); }
                    if (e.r2) { const uint2 t = *(const uint2*)(e.r2 + pix * e.ldr2 + n0); r2v[0] = bf16lo(t.x); r2v[1] = bf16hi(t.x); r2v[2] = bf16lo(t.y); r2v[3] = bf16hi(t.y); }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (n0 + j < p.N_live) {
                            if (e.r1) r1v[j] = bf16_to_f32(e.r1[pix * e.ldr1 + n0 + j]);
                            if (e.r2) r2v[j] = bf16_to_f32(e.r2[pix * e.ldr2 + n0 + j]);
                        }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float b = (e.bias && n0 + j < p.N_live) ? e.bias[n0 + j] : 0.f;
                    v[j] = rdb_epilogue_value(acc[m][nb][4 * g + j], b, e.alpha, e.act, e.r1 != nullptr, r1v[j], e.beta1, e.r2 != nullptr, r2v[j], e.beta2);
                }
                bf16_t* dst = p.out + pix * p.ldo + n0;
                if (full) {
                    uint2 o; o.x = pack_bf16x2(v[0], v[1]); o.y = pack_bf16x2(v[2], v[3]);
                    *(uint2*)dst = o;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (n0 + j < p.N_live) dst[j] = f32_to_bf16(v[j]);
                }
            }
    }
}

// wd[kc][tap][n][c] = n < rows ? W[n][tap * Cin + kc * 32 + c] : 0     (W: the library's conv layout [rows][9][Cin]); 8 elements per lane
__global__ void k_rdb_wpack(const bf16_t* __restrict__ W, int rows, int Cin, int NT, bf16_t* __restrict__ wd, size_t total8) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total8) return;
    const int c8 = (int)(i & 3), n = (int)((i >> 2) % NT), tap = (int)((i / (4 * (size_t)NT)) % 9), kc = (int)(i / (36 * (size_t)NT));
    uint4 v = {0u, 0u, 0u, 0u};
    if (n < rows) v = *(const uint4*)(W + ((size_t)n * 9 + tap) * Cin + kc * RDB_KC + c8 * 8);
    ((uint4*)wd)[i] = v;
}

size_t rdb_wpack_bytes(int NT, int Cin) { return (size_t)NT * 9 * Cin * sizeof(bf16_t); }
void rdb_tile(int* th, int* tw) { *th = RDB_TH; *tw = RDB_TW; }

int launch_rdb_wpack(hipStream_t st, const bf16_t* W, int rows, int Cin, int NT, bf16_t* wd) {
    if (!W || !wd) GYRE_FAIL(GYRE_ERR_INVALID, "rdb_wpack: null argument");
    if (NT != 32 && NT != 64) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "rdb_wpack: NT must be 32 or 64");
    if (Cin < RDB_KC || Cin % RDB_KC) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "rdb_wpack: Cin must be a positive multiple of 32");
    if (rows < 1 || rows > NT) GYRE_FAIL(GYRE_ERR_INVALID, "rdb_wpack: 1 to NT weight rows");
    if (((size_t)W | (size_t)wd) & 15) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "rdb_wpack: 16-byte aligned buffers");
    const size_t total8 = (size_t)NT * 9 * Cin / 8;
    hipLaunchKernelGGL(k_rdb_wpack, dim3((unsigned)((total8 + 255) / 256)), dim3(256), 0, st, W, rows, Cin, NT, wd, total8);
    GYRE_LAUNCH_CHECK();
    return 0;
}

static int rdb_check_epilogue(const char* who, const RdbEpilogueArgs& e, int N_live) {
    if (!std::isfinite(e.alpha) || !std::isfinite(e.beta1) || !std::isfinite(e.beta2)) GYRE_FAIL(GYRE_ERR_INVALID, std::string(who) + ": alpha / beta must be finite");
    if (N_live < 1) GYRE_FAIL(GYRE_ERR_INVALID, std::string(who) + ": N_live must be positive");
    if ((e.r1 && e.ldr1 < N_live) || (e.r2 && e.ldr2 < N_live)) GYRE_FAIL(GYRE_ERR_INVALID, std::string(who) + ": a residual's pixel stride is below N_live");
    if ((e.r1 && (e.ldr1 % 8 || ((size_t)e.r1 & 15))) || (e.r2 && (e.ldr2 % 8 || ((size_t)e.r2 & 15))))
        GYRE_FAIL(GYRE_ERR_UNSUPPORTED, std::string(who) + ": residual slices need 16-byte alignment and a pixel stride that is a multiple of 8");
    return 0;
}

// every refusal of launch_rdb_conv, without a device call (gyre_op_rdb_conv asks before it touches its weight scratch)
int rdb_conv_check(const bf16_t* x, int ldx, int Cin, int B, int H, int W, int ups, const bf16_t* wd, int NT, int N_live,
                   const bf16_t* out, int ldo, const RdbEpilogueArgs& e) {
    if (!x || !wd || !out) GYRE_FAIL(GYRE_ERR_INVALID, "rdb_conv: null argument");
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || ldx < Cin) GYRE_FAIL(GYRE_ERR_INVALID, "rdb_conv: bad sizes (B, H, W, Cin positive, ldx >= Cin)");
    if (NT != 32 && NT != 64) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "rdb_conv: NT must be 32 or 64");
    if (N_live < 1 || N_live > NT || ldo < N_live) GYRE_FAIL(GYRE_ERR_INVALID, "rdb_conv: 1 <= N_live <= NT and ldo >= N_live");
    RDB_TRY(rdb_check_epilogue("rdb_conv", e, N_live));
    if (Cin % RDB_KC) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "rdb_conv: Cin must be a multiple of 32");
    if (ldx % 8 || ldo % 8 || (((size_t)x | (size_t)wd | (size_t)out) & 15))
        GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "rdb_conv: pixel strides must be multiples of 8 elements and the slices 16-byte aligned");
    const int Ho = ups ? 2 * H : H, Wo = ups ? 2 * W : W;
    const size_t tiles = (size_t)((Ho + RDB_TH - 1) / RDB_TH) * ((Wo + RDB_TW - 1) / RDB_TW);
    if (B > 65535 || tiles >= (1ull << 31) || (size_t)H * W * ldx >= (1ull << 31) || (size_t)B * Ho * Wo >= (1ull << 31))
        GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "rdb_conv: grid limits (B <= 65535, a sample below 2^31 elements, fewer than 2^31 output pixels)");
    return 0;
}

int launch_rdb_conv(hipStream_t st, const bf16_t* x, int ldx, int Cin, int B, int H, int W, int ups, const bf16_t* wd, int NT,
                    int N_live, bf16_t* out, int ldo, const RdbEpilogueArgs& e) {
    RDB_TRY(rdb_conv_check(x, ldx, Cin, B, H, W, ups, wd, NT, N_live, out, ldo, e));
    const int Ho = ups ? 2 * H : H, Wo = ups ? 2 * W : W;
    const size_t tiles = (size_t)((Ho + RDB_TH - 1) / RDB_TH) * ((Wo + RDB_TW - 1) / RDB_TW);
    RdbConvParams p;
    p.x = x; p.ldx = ldx; p.Cin = Cin; p.H = H; p.W = W; p.ups = ups ? 1 : 0; p.wd = wd; p.out = out; p.ldo = ldo; p.N_live = N_live;
    p.e.bias = e.bias; p.e.alpha = e.alpha; p.e.act = e.act ? 1 : 0;
    p.e.r1 = e.r1; p.e.ldr1 = e.ldr1; p.e.beta1 = e.beta1; p.e.r2 = e.r2; p.e.ldr2 = e.ldr2; p.e.beta2 = e.beta2;
    const size_t lds = (size_t)RDB_HALO * 64 + (size_t)9 * NT * 64;
    static std::atomic<unsigned long long> done32{0}, done64{0};
    const double flops = 2.0 * B * Ho * Wo * NT * 9.0 * Cin, bytes = (double)B * H * W * Cin * 2 + (double)B * Ho * Wo * N_live * 2;
    GyreProfScope prof(KC_OTHER, st, flops, bytes);
    if (NT == 32) {
        if (gyre_lds_attr_needed(done32)) GYRE_HIP_CHECK(hipFuncSetAttribute((const void*)k_rdb_conv<32>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_rdb_conv<32>, dim3((unsigned)tiles, (unsigned)B), dim3(256), lds, st, p);
    } else {
        if (gyre_lds_attr_needed(done64)) GYRE_HIP_CHECK(hipFuncSetAttribute((const void*)k_rdb_conv<64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_rdb_conv<64>, dim3((unsigned)tiles, (unsigned)B), dim3(256), lds, st, p);
    }
    GYRE_LAUNCH_CHECK();
    return 0;
}

// In place over the slice x[pix][0 .. N_live) (x: first element of the slice, pixel stride ldo): one lane per (pixel, 8 channels)
__global__ void k_rdb_epilogue(bf16_t* __restrict__ x, int ldo, int N_live, size_t npix, RdbEpi e) {
    const int G = (N_live + 7) / 8;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix * G) return;
    const size_t pix = i / G;
    const int n0 = (int)(i % G) * 8;
    bf16_t* dst = x + pix * ldo + n0;
    float v[8], r1v[8], r2v[8];
    if (n0 + 8 <= N_live) {
        unpack8(*(const uint4*)dst, v);
        if (e.r1) unpack8(*(const uint4*)(e.r1 + pix * e.ldr1 + n0), r1v);
        if (e.r2) unpack8(*(const uint4*)(e.r2 + pix * e.ldr2 + n0), r2v);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            v[j] = rdb_epilogue_value(v[j], e.bias ? e.bias[n0 + j] : 0.f, e.alpha, e.act, e.r1 != nullptr, e.r1 ? r1v[j] : 0.f, e.beta1,
                                      e.r2 != nullptr, e.r2 ? r2v[j] : 0.f, e.beta2);
        *(uint4*)dst = pack8(v);
    } else {
        for (int j = 0; n0 + j < N_live; ++j) {
            const float a = bf16_to_f32(dst[j]);
            const float q1 = e.r1 ? bf16_to_f32(e.r1[pix * e.ldr1 + n0 + j]) : 0.f, q2 = e.r2 ? bf16_to_f32(e.r2[pix * e.ldr2 + n0 + j]) : 0.f;
            dst[j] = f32_to_bf16(rdb_epilogue_value(a, e.bias ? e.bias[n0 + j] : 0.f, e.alpha, e.act, e.r1 != nullptr, q1, e.beta1,
                                                    e.r2 != nullptr, q2, e.beta2));
        }
    }
}
int launch_rdb_epilogue(hipStream_t st, bf16_t* x, int ldo, int N_live, size_t npix, const RdbEpilogueArgs& e) {
    if (!x) GYRE_FAIL(GYRE_ERR_INVALID, "rdb_epilogue: null argument");
    if (npix < 1 || ldo < N_live) GYRE_FAIL(GYRE_ERR_INVALID, "rdb_epilogue: bad sizes");
    RDB_TRY(rdb_check_epilogue("rdb_epilogue", e, N_live));
    if (ldo % 8 || ((size_t)x & 15)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "rdb_epilogue: the slice needs 16-byte alignment and a pixel stride that is a multiple of 8");
    const size_t total = npix * ((N_live + 7) / 8);
    if (total >= (1ull << 31) * 256) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "rdb_epilogue: grid limits");
    RdbEpi d;
    d.bias = e.bias; d.alpha = e.alpha; d.act = e.act ? 1 : 0; d.r1 = e.r1; d.ldr1 = e.ldr1; d.beta1 = e.beta1; d.r2 = e.r2; d.ldr2 = e.ldr2; d.beta2 = e.beta2;
    hipLaunchKernelGGL(k_rdb_epilogue, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, ldo, N_live, npix, d);
    GYRE_LAUNCH_CHECK();
    return 0;
}

// x NCHW [B][c][H][W] (runtime dtype) -> y NHWC storage [B][H / r][W / r][Cpad], Cpad = c r^2 rounded up to 32, channel
// ci r^2 + dy r + dx (torch.nn.functional.pixel_unshuffle), zeros above c r^2.  One lane per (pixel, 8 channels).
__global__ void k_pixel_unshuffle(const void* __restrict__ x, int dtype, int c, int H, int W, int r, int Cpad, bf16_t* __restrict__ y, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int G = Cpad / 8, Ho = H / r, Wo = W / r, rr = r * r;
    const int g = (int)(i % G);
    const size_t pix = i / G;
    const size_t wo = pix % Wo, ho = (pix / Wo) % Ho, b = pix / ((size_t)Wo * Ho);
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ch = g * 8 + j;
        f[j] = 0.f;
        if (ch < c * rr) {
            const int ci = ch / rr, dy = (ch % rr) / r, dx = ch % r;
            f[j] = load_as_f32(x, dtype, ((b * c + ci) * H + ho * r + dy) * W + wo * r + dx);
        }
    }
    *(uint4*)(y + i * 8) = pack8(f);
}
int rdb_unshuffle_channels(int c, int r) { return (c * r * r + 31) / 32 * 32; }
int launch_pixel_unshuffle(hipStream_t st, const void* x, int dtype, int B, int c, int H, int W, int r, bf16_t* y) {
    if (!x || !y) GYRE_FAIL(GYRE_ERR_INVALID, "pixel_unshuffle: null argument");
    if (r != 1 && r != 2 && r != 4) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "pixel_unshuffle: r must be 1, 2 or 4");
    if (dtype < 0 || dtype > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    if (B < 1 || c < 1 || H < r || W < r || H % r || W % r) GYRE_FAIL(GYRE_ERR_INVALID, "pixel_unshuffle: H and W must be positive multiples of r");
    const int Cpad = rdb_unshuffle_channels(c, r);
    const size_t total = (size_t)B * (H / r) * (W / r) * (Cpad / 8);
    if (total >= (1ull << 31) * 256) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "pixel_unshuffle: grid limits");
    hipLaunchKernelGGL(k_pixel_unshuffle, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, dtype, c, H, W, r, Cpad, y, total);
    GYRE_LAUNCH_CHECK();
    return 0;
}

// dst[pix][0 .. C) = src[pix][0 .. C)  (C % 8 == 0, pixel strides ldd / lds, 16 bytes per lane): the RRDB input kept aside
__global__ void k_rdb_copy(const bf16_t* __restrict__ src, int lds, bf16_t* __restrict__ dst, int ldd, int C8, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t pix = i / C8, c = (i % C8) * 8;
    *(uint4*)(dst + pix * ldd + c) = *(const uint4*)(src + pix * lds + c);
}
int launch_rdb_copy(hipStream_t st, const bf16_t* src, int lds, bf16_t* dst, int ldd, int C, size_t npix) {
    if (!src || !dst) GYRE_FAIL(GYRE_ERR_INVALID, "rdb_copy: null argument");
    if (C < 8 || C % 8 || lds % 8 || ldd % 8 || lds < C || ldd < C || npix < 1 || (((size_t)src | (size_t)dst) & 15))
        GYRE_FAIL(GYRE_ERR_INVALID, "rdb_copy: C and the strides must be multiples of 8 and the slices 16-byte aligned");
    const size_t total = npix * (C / 8);
    if (total >= (1ull << 31) * 256) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "rdb_copy: grid limits");
    hipLaunchKernelGGL(k_rdb_copy, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, lds, dst, ldd, C / 8, total);
    GYRE_LAUNCH_CHECK();
    return 0;
}
