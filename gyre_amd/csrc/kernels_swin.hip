// SwinIR kernels: shifted-window attention over 8 x 8 windows and the small passes the RSTB graph needs (model_swinir.hip).
//
// k_win_attn - one WAVE per (sample, window, head), four waves (four neighbouring heads of the same window where there are that many)
// per workgroup, no LDS.  The 64 tokens of a window are addressed in place: token (i, j) of window (wy, wx) under shift s is the
// image pixel ((8 wy + i + s) mod H, (8 wx + j + s) mod W), for the q / k / v reads and for the store alike, so neither the rolled nor
// the window-partitioned tensor of the reference (network_swinir.py:253-278) ever exists.
//
//   qkv [B H W][ld_qkv]   fused projection output in token order; q of head h at columns [32 h, 32 h + 32), k at 32 (heads + h),
//                         v at 32 (2 heads + h): 30 live columns and 2 the weight repack keeps exactly zero
//   o   [B H W][ld_o]     head h at columns [30 h, 30 h + 30); no other column is written
//
// Arithmetic, per (window, head), for query a and key b (a = 8 i + j):
//   l[a][b] = scale * sum_d q[a][d] k[b][d] + bias[h][a][b] + (s > 0 and id(a) != id(b) ? -100 : 0)       fp32; scale = 30^-1/2 (an fp32 constant),
//                                                                                                       applied to the fp32 dot product, NOT folded into the weights
//   p[a][b] = exp(l[a][b] - max_b l[a][.]) / sum_b exp(..)      fp32, whole 64-wide row in registers; rounded ONCE to storage
//   o[a][d] = sum_b p[a][b] v[b][d]                            fp32 accumulation, rounded once to storage
// id = 3 r(8 wy + i, H) + r(8 wx + j, W), r(Y, L) = 0 if Y < L - 8, 1 if Y < L - s, else 2: SwinTransformerBlock.calculate_mask
// computed from the window position, no mask tensor is read.
//
// MFMA plan (v_mfma_f32_32x32x16).  The logits are produced TRANSPOSED, X = K Q^T (rows = keys, columns = queries): both operands
// are then 16-byte row reads of the qkv rows (A: lane (r, h) holds k[key r][16 t + 8 h ..+8], B: q[query r][same columns]), and
// a lane ends up holding one query column with its keys in the 16 accumulator registers of each 32 x 32 tile - key
// 32 kt + (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  A softmax row is therefore the lane's own 32 registers plus those of lane ^ 32:
// one cross-lane exchange per reduction.  The normalised, rounded P^T tile is the A operand of the second product without any lane
// movement (registers 8 t .. 8 t + 7 are k-step t; element j of lane half h is key 32 kt + 16 t + 8 (j >> 2) + 4 h + (j & 3)), and the B
// operand gathers v[that key][d = lane & 31] with 2-byte loads: 32 lanes of a half read one 64-byte row segment per load.  The result
// tile has d on the lane and the query in the registers, so each store instruction writes 60 contiguous bytes per half wave.
// Every global access of the kernel is a 64-byte (60 for the store) segment of one token row.
//
// The expanded bias (launch_win_bias) is stored in this register order, [head][query tile][key tile][reg >> 2][lane][reg & 3] fp32,
// so the kernel reads it as one coalesced 16-byte load per four registers.
#include "kernels.h"
#include "../../include/gyre_hip.h"
#include <algorithm>
#include <cmath>

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

namespace {
struct WinAttnParams {
    const bf16_t* qkv; int ld_qkv;
    bf16_t* o; int ld_o;
    const float* bias;            // [heads][4096] in register order
    int B, H, W, heads, shift;
    unsigned total;               // B * (H / 8) * (W / 8) * heads waves
};

__device__ __forceinline__ int swin_region(int Y, int L, int s) { return Y < L - 8 ? 0 : (Y < L - s ? 1 : 2); }

__global__ __launch_bounds__(256) void k_win_attn(WinAttnParams p) {
    const int lane = threadIdx.x & 63;
    const unsigned wv = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (wv >= p.total) return;
    const int nwx = p.W >> 3, nwy = p.H >> 3;
    const int head = (int)(wv % (unsigned)p.heads);
    unsigned rest = wv / (unsigned)p.heads;
    const int wx = (int)(rest % (unsigned)nwx); rest /= (unsigned)nwx;
    const int wy = (int)(rest % (unsigned)nwy);
    const int b = (int)(rest / (unsigned)nwy);
    const int s = p.shift;
    const int r = lane & 31, hh = lane >> 5;
    const size_t img0 = (size_t)b * p.H * p.W;
    // token t (0 .. 63) of this window -> row of the token-order tensors
    auto tok_row = [&](int t) -> size_t {
        int y = 8 * wy + (t >> 3) + s; if (y >= p.H) y -= p.H;
        int x = 8 * wx + (t & 7) + s;  if (x >= p.W) x -= p.W;
        return img0 + (size_t)y * p.W + x;
    };
    auto tok_id = [&](int t) -> int { return 3 * swin_region(8 * wy + (t >> 3), p.H, s) + swin_region(8 * wx + (t & 7), p.W, s); };
    const bf16_t* qb = p.qkv + 32 * head;
    const bf16_t* kb = p.qkv + 32 * (p.heads + head);
    const bf16_t* vb = p.qkv + 32 * (2 * p.heads + head);

    // K fragments (A operand of X = K Q^T): [key tile][k-step]
    bf16x8_t kf[2][2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        const bf16_t* row = kb + tok_row(32 * kt + r) * p.ld_qkv + 8 * hh;
        kf[kt][0] = *(const bf16x8_t*)(row);
        kf[kt][1] = *(const bf16x8_t*)(row + 16);
    }
    // V fragments (B operand of O = P V): [key tile][k-step], element j = v[key 32 kt + 16 t + 8 (j >> 2) + 4 hh + (j & 3)][d = r]
    bf16x8_t vf[2][2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            uint32_t w[4];
#pragma unroll
            for (int jp = 0; jp < 4; ++jp) {
                const int j0 = 2 * jp;
                const int key0 = 32 * kt + 16 * t + 8 * (j0 >> 2) + 4 * hh + (j0 & 3);
                const uint32_t lo = vb[tok_row(key0) * p.ld_qkv + r], hi = vb[tok_row(key0 + 1) * p.ld_qkv + r];
                w[jp] = lo | (hi << 16);
            }
            uint4 u = {w[0], w[1], w[2], w[3]};
            vf[kt][t] = __builtin_bit_cast(bf16x8_t, u);
        }
    const float scale = 0.18257418583505536f;            // 30^-1/2
    const float4* bias4 = (const float4*)(p.bias + (size_t)head * 4096);

#pragma unroll 1
    for (int qt = 0; qt < 2; ++qt) {
        const int qtok = 32 * qt + r;
        const size_t qrow = tok_row(qtok);
        const bf16_t* qp = qb + qrow * p.ld_qkv + 8 * hh;
        const bf16x8_t q0 = *(const bf16x8_t*)(qp), q1 = *(const bf16x8_t*)(qp + 16);
        const int qid = s ? tok_id(qtok) : 0;
        f32x16_t x[2];
        float m = -3.0e38f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            f32x16_t acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            acc = GYRE_MFMA_32x32x16(kf[kt][0], q0, acc, 0, 0, 0);
            acc = GYRE_MFMA_32x32x16(kf[kt][1], q1, acc, 0, 0, 0);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 bv = bias4[((qt * 2 + kt) * 4 + g) * 64 + lane];
                const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int key = 32 * kt + 8 * g + 4 * hh + i;
                    float l = fmaf(scale, acc[4 * g + i], bb[i]);
                    if (s && tok_id(key) != qid) l += -100.f;
                    acc[4 * g + i] = l;
                    m = fmaxf(m, l);
                }
            }
            x[kt] = acc;
        }
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float e = __expf(x[kt][i] - m);
                x[kt][i] = e;
                sum += e;
            }
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.0f / sum;
        f32x16_t oacc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                uint4 u;
                u.x = pack_bf16x2(x[kt][8 * t + 0] * inv, x[kt][8 * t + 1] * inv);
                u.y = pack_bf16x2(x[kt][8 * t + 2] * inv, x[kt][8 * t + 3] * inv);
                u.z = pack_bf16x2(x[kt][8 * t + 4] * inv, x[kt][8 * t + 5] * inv);
                u.w = pack_bf16x2(x[kt][8 * t + 6] * inv, x[kt][8 * t + 7] * inv);
                oacc = GYRE_MFMA_32x32x16(__builtin_bit_cast(bf16x8_t, u), vf[kt][t], oacc, 0, 0, 0);
            }
        // tile [query 32 qt + (reg & 3) + 8 (reg >> 2) + 4 hh][d = r]
        if (r < 30) {
            bf16_t* ob = p.o + 30 * head + r;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int tq = 32 * qt + (i & 3) + 8 * (i >> 2) + 4 * hh;
                ob[tok_row(tq) * p.ld_o] = f32_to_bf16(oacc[i]);
            }
        }
    }
}

// table [225][heads] fp32 -> the kernel's register order (header): bias[h][a][b] = table[(i - i' + 7) * 15 + (j - j' + 7)][h]
__global__ void k_win_bias(const float* __restrict__ table, int heads, float* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= heads * 4096) return;
    const int i = idx & 3, lane = (idx >> 2) & 63, g = (idx >> 8) & 3, kt = (idx >> 10) & 1, qt = (idx >> 11) & 1, h = idx >> 12;
    const int a = 32 * qt + (lane & 31), b = 32 * kt + 8 * g + 4 * (lane >> 5) + i;
    const int di = (a >> 3) - (b >> 3) + 7, dj = (a & 7) - (b & 7) + 7;
    out[idx] = table[(di * 15 + dj) * heads + h];
}

// LayerNorm over the first C channels of rows of stride ldx; y rows of stride ldy: the normalised values in [0, C), zeros in [C, ldy).
// One wave per row at a time, the row in registers (C, ldy <= 512), two-pass variance, fp32, one rounding.  Lane l holds the channel
// quads [4 l, 4 l + 4) and [256 + 4 l, ..): VEC (strides multiples of 4, 8-byte aligned rows) moves a whole quad with one 8-byte
// access, the other form element by element; the arithmetic and its order are the same.  A wave walks rows w, w + waves, ... with the
// next row's loads issued before the current row's reductions, gamma / beta held in registers: a grid of one short-lived wave per
// 384-byte row was bound by the rate waves can be started at, not by memory.
template <bool VEC>
__device__ __forceinline__ void ln_load_row(const bf16_t* __restrict__ xr, int C, int lane, float* v) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c0 = 4 * lane + 256 * i;
        if (VEC && c0 + 4 <= C) {
            const uint2 w = *(const uint2*)(xr + c0);
            v[4 * i + 0] = bf16lo(w.x); v[4 * i + 1] = bf16hi(w.x); v[4 * i + 2] = bf16lo(w.y); v[4 * i + 3] = bf16hi(w.y);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * i + j] = c0 + j < C ? bf16_to_f32(xr[c0 + j]) : 0.f;
        }
    }
}
template <bool VEC>
__global__ __launch_bounds__(256) void k_ln_live(const bf16_t* __restrict__ x, int ldx, size_t M, int C, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, float eps, bf16_t* __restrict__ y, int ldy) {
    const int lane = threadIdx.x & 63;
    const size_t nwaves = (size_t)gridDim.x * 4;
    size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float g[8], bt[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = 4 * lane + 256 * (i >> 2) + (i & 3);
        g[i] = c < C ? gamma[c] : 0.f;
        bt[i] = c < C ? beta[c] : 0.f;
    }
    float v[8], vn[8];
    ln_load_row<VEC>(x + row * ldx, C, lane, v);
    while (true) {
        const size_t next = row + nwaves;
        if (next < M) ln_load_row<VEC>(x + next * ldx, C, lane, vn);
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) sum += v[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        const float mean = sum / (float)C;
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = 4 * lane + 256 * (i >> 2) + (i & 3);
            const float d = c < C ? v[i] - mean : 0.f;
            sq = fmaf(d, d, sq);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
        const float rstd = 1.0f / sqrtf(sq / (float)C + eps);
        bf16_t* yr = y + row * ldy;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c0 = 4 * lane + 256 * i;
            float o4[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o4[j] = c0 + j < C ? fmaf((v[4 * i + j] - mean) * rstd, g[4 * i + j], bt[4 * i + j]) : 0.f;
            if (VEC && c0 + 4 <= ldy) {
                uint2 w;
                w.x = pack_bf16x2(o4[0], o4[1]); w.y = pack_bf16x2(o4[2], o4[3]);
                *(uint2*)(yr + c0) = w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c0 + j < ldy) yr[c0 + j] = f32_to_bf16(o4[j]);
            }
        }
        if (next >= M) break;
        row = next;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = vn[i];
    }
}

// in place over n contiguous elements (n % 8 == 0): mode 0 = erf GELU (0.5 x (1 + erf(x / sqrt 2)), libm erff), 1 = x > 0 ? x : slope x
__global__ void k_swin_act(bf16_t* __restrict__ x, size_t n8, int mode, float slope) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    float f[8];
    unpack8(*(const uint4*)(x + i * 8), f);
#pragma unroll
    for (int j = 0; j < 8; ++j)
        f[j] = mode == 0 ? 0.5f * f[j] * (1.0f + erff(f[j] * 0.70710678118654752f)) : (f[j] > 0.f ? f[j] : slope * f[j]);
    *(uint4*)(x + i * 8) = pack8(f);
}

// x NCHW [B][3][HW] of a runtime dtype -> y NHWC storage [B][HW][8]: (x - mean[c]) * range in channels 0 .. 2, zeros above
__global__ void k_swin_entry(const void* __restrict__ x, int dtype, size_t HW, size_t total, float m0, float m1, float m2, float range,
                             bf16_t* __restrict__ y) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / HW, pix = i % HW;
    const float mean[3] = {m0, m1, m2};
    float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c) f[c] = (load_as_f32(x, dtype, (b * 3 + c) * HW + pix) - mean[c]) * range;
    *(uint4*)(y + i * 8) = pack8(f);
}
// x NHWC storage [B][HW][ldx] -> y NCHW [B][3][HW] of a runtime dtype: x / range + mean[c]
__global__ void k_swin_exit(const bf16_t* __restrict__ x, int ldx, size_t HW, size_t total, float m0, float m1, float m2, float range,
                            void* __restrict__ y, int dtype) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / HW, pix = i % HW;
    const float mean[3] = {m0, m1, m2};
#pragma unroll
    for (int c = 0; c < 3; ++c) store_from_f32(y, dtype, (b * 3 + c) * HW + pix, bf16_to_f32(x[i * ldx + c]) / range + mean[c]);
}
}  // namespace

int win_attn_check(const bf16_t* qkv, int ld_qkv, const bf16_t* o, int ld_o, const float* bias, int B, int H, int W, int heads, int shift) {
    if (!qkv || !o || !bias) GYRE_FAIL(GYRE_ERR_INVALID, "win_attn: null argument");
    if (B < 1 || H < 8 || W < 8 || H % 8 || W % 8) GYRE_FAIL(GYRE_ERR_INVALID, "win_attn: H and W must be multiples of the window size 8");
    if (heads < 1 || heads > 8) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "win_attn: 1 to 8 heads of 30 channels are built");
    if (shift != 0 && shift != 4) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "win_attn: the shift is 0 or half the window (4)");
    if (shift && (H == 8 || W == 8)) GYRE_FAIL(GYRE_ERR_INVALID, "win_attn: an image of one window per side is not shifted");
    if (ld_qkv < 96 * heads || ld_o < 30 * heads) GYRE_FAIL(GYRE_ERR_INVALID, "win_attn: row strides below 96 heads (qkv) / 30 heads (o)");
    if (ld_qkv % 8 || ((size_t)qkv & 15) || ((size_t)bias & 15) || ((size_t)o & 1))
        GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "win_attn: qkv needs 16-byte aligned rows (stride a multiple of 8) and a 16-byte aligned bias");
    if ((size_t)B * (H / 8) * (W / 8) * heads >= (1ull << 31)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "win_attn: grid limits");
    return 0;
}
int launch_win_attn(hipStream_t st, const bf16_t* qkv, int ld_qkv, bf16_t* o, int ld_o, const float* bias, int B, int H, int W, int heads,
                    int shift) {
    int rc = win_attn_check(qkv, ld_qkv, o, ld_o, bias, B, H, W, heads, shift);
    if (rc) return rc;
    WinAttnParams p;
    p.qkv = qkv; p.ld_qkv = ld_qkv; p.o = o; p.ld_o = ld_o; p.bias = bias; p.B = B; p.H = H; p.W = W; p.heads = heads; p.shift = shift;
    p.total = (unsigned)((size_t)B * (H / 8) * (W / 8) * heads);
    const double pairs = (double)p.total;
    GyreProfScope prof(KC_ATTN, st, pairs * 2.0 * 2.0 * 64 * 64 * 32, pairs * (3.0 * 64 * 64 + 64 * 60));
    hipLaunchKernelGGL(k_win_attn, dim3((p.total + 3) / 4), dim3(256), 0, st, p);
    GYRE_LAUNCH_CHECK();
    return 0;
}
int launch_win_bias(hipStream_t st, const float* table, int heads, float* out) {
    if (!table || !out) GYRE_FAIL(GYRE_ERR_INVALID, "win_bias: null argument");
    if (heads < 1 || heads > 8) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "win_bias: 1 to 8 heads");
    hipLaunchKernelGGL(k_win_bias, dim3(heads * 16), dim3(256), 0, st, table, heads, out);
    GYRE_LAUNCH_CHECK();
    return 0;
}
int launch_ln_live(hipStream_t st, const bf16_t* x, int ldx, size_t M, int C, const float* gamma, const float* beta, float eps, bf16_t* y,
                   int ldy) {
    if (!x || !y || !gamma || !beta) GYRE_FAIL(GYRE_ERR_INVALID, "ln_live: null argument");
    if (M < 1 || C < 1 || ldx < C || ldy < C) GYRE_FAIL(GYRE_ERR_INVALID, "ln_live: the row strides must cover the C live channels");
    if (C > 512 || ldy > 512) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "ln_live: at most 512 channels per row");
    GyreProfScope prof(KC_LAYERNORM, st, 8.0 * M * C, 4.0 * M * C);
    const bool vec = ldx % 4 == 0 && ldy % 4 == 0 && !(((size_t)x | (size_t)y) & 7);
    const unsigned blocks = (unsigned)std::min<size_t>((M + 3) / 4, 4096);      // at most 16 K waves, each walking its rows
    if (vec) hipLaunchKernelGGL(k_ln_live<true>, dim3(blocks), dim3(256), 0, st, x, ldx, M, C, gamma, beta, eps, y, ldy);
    else hipLaunchKernelGGL(k_ln_live<false>, dim3(blocks), dim3(256), 0, st, x, ldx, M, C, gamma, beta, eps, y, ldy);
    GYRE_LAUNCH_CHECK();
    return 0;
}
int launch_swin_act(hipStream_t st, bf16_t* x, size_t n, int mode, float slope) {
    if (!x) GYRE_FAIL(GYRE_ERR_INVALID, "swin_act: null argument");
    if (mode != 0 && mode != 1) GYRE_FAIL(GYRE_ERR_INVALID, "swin_act: mode 0 (erf GELU) or 1 (leaky ReLU)");
    if (n < 8 || n % 8 || ((size_t)x & 15)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swin_act: a 16-byte aligned buffer of a multiple of 8 elements");
    if (n / 8 >= (1ull << 31) * 256) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swin_act: grid limits");
    GyreProfScope prof(KC_OTHER, st, (double)n, 4.0 * n);
    hipLaunchKernelGGL(k_swin_act, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, st, x, n / 8, mode, slope);
    GYRE_LAUNCH_CHECK();
    return 0;
}
int launch_swin_entry(hipStream_t st, const void* x, int dtype, int B, size_t HW, const float* mean3, float range, bf16_t* y) {
    if (!x || !y || !mean3) GYRE_FAIL(GYRE_ERR_INVALID, "swin_entry: null argument");
    if (dtype < 0 || dtype > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    if (B < 1 || HW < 1 || ((size_t)y & 15)) GYRE_FAIL(GYRE_ERR_INVALID, "swin_entry: bad sizes or an unaligned output");
    const size_t total = (size_t)B * HW;
    if (total >= (1ull << 31) * 256) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swin_entry: grid limits");
    hipLaunchKernelGGL(k_swin_entry, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, dtype, HW, total, mean3[0], mean3[1], mean3[2],
                       range, y);
    GYRE_LAUNCH_CHECK();
    return 0;
}
int launch_swin_exit(hipStream_t st, const bf16_t* x, int ldx, int B, size_t HW, const float* mean3, float range, void* y, int dtype) {
    if (!x || !y || !mean3) GYRE_FAIL(GYRE_ERR_INVALID, "swin_exit: null argument");
    if (dtype < 0 || dtype > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    if (B < 1 || HW < 1 || ldx < 3 || range == 0.f) GYRE_FAIL(GYRE_ERR_INVALID, "swin_exit: bad sizes");
    const size_t total = (size_t)B * HW;
    if (total >= (1ull << 31) * 256) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swin_exit: grid limits");
    hipLaunchKernelGGL(k_swin_exit, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, ldx, HW, total, mean3[0], mean3[1], mean3[2], range,
                       y, dtype);
    GYRE_LAUNCH_CHECK();
    return 0;
}
