// HAT kernels: attention over 16 x 16 windows (self-attention and the overlapping cross-attention), the channel-attention passes of the
// CAB (pool, gate, scale-add) and PixelShuffle(2) on NHWC (model_hat.hip).
//
// k_hat_attn<OCA> - one 256-thread workgroup per (sample, window, head); wave w owns the queries [64 w, 64 w + 64) of the window as two
// 32-query tiles.  The tokens are addressed in place, as in k_win_attn (kernels_swin.hip): no rolled, partitioned or unfolded tensor exists.
//
//   qkv [B H W][ld_qkv]   fused projection output in token order; q of head h at columns [32 h, 32 h + 32), k at 32 (heads + h),
//                         v at 32 (2 heads + h): 30 live columns and 2 the weight repack keeps exactly zero
//   o   [B H W][ld_o]     head h at columns [30 h, 30 h + 30); no other column is written
//   table                 the relative-position table, fp32 [961][heads] (SA) / [1521][heads] (OCA)
//
// SA  (OCA = false): query a = 16 i + j and key b = 16 i' + j' of window (wy, wx) under shift s (0 or 8) are the pixels
//     ((16 wy + i + s) mod H, (16 wx + j + s) mod W);  bias = table[(i - i' + 15) 31 + (j - j' + 15)];  for s > 0 the mask -100 where
//     id(a) != id(b), id = 3 r(16 wy + i, H) + r(16 wx + j, W), r(Y, L) = 0 if Y < L - 16, 1 if Y < L - 8, else 2 (HAT.calculate_mask from
//     the window position; the shift is applied whatever the image size, as the reference builds its blocks for img_size 64).
// OCA (OCA = true):  query (i, j) is pixel (16 wy + i, 16 wx + j); key (ey, ex), 0 <= ey, ex < 24, is pixel (16 wy - 4 + ey, 16 wx - 4 + ex);
//     a key outside the image has k = v = 0 (nn.Unfold pads after the projection) and still takes part in the softmax with logit = its
//     bias;  bias = table[((ey - i - 7) 39 + (ex - j - 7)) mod 1521] - the reference's index is negative for most pairs and wraps through
//     negative indexing; no mask, no shift.
//
// Arithmetic, per query a over the nk = 256 / 576 keys:
//   l[a][b] = scale * sum_d q[a][d] k[b][d] + bias (+ mask)     fp32; scale = 30^-1/2 (an fp32 constant) applied to the fp32 dot product
//   p[a][b] = exp(l[a][b] - M[a]) / S[a]                        fp32, rounded ONCE to storage
//   o[a][d] = sum_b p[a][b] v[b][d]                             fp32 accumulation, rounded once to storage
// A row of 576 logits does not fit the registers, so the logits are computed twice.  Pass 1 keeps, per lane, a running maximum m and the
// sum of exp(l - m), rescaled by exp(m_old - m_new) when a 32-key tile raises the maximum (at most nk / 32 rescalings), and merges the two
// lanes of a query at the end: M is the exact row maximum, S the row sum of exp(l - M) up to those rescalings.  Pass 2 recomputes the same
// logits (the same instructions on the same operands: the same bits), forms p = exp(l - M) * (1 / S), rounds it and multiplies by V.
//
// LDS.  K rows [nk][40] storage (80-byte pitch: the 16-byte fragment reads of 32 consecutive rows fall on distinct bank groups), V
// TRANSPOSED [32][nk + 4] (pitch 520 / 1160 bytes), written element-wise at staging time so that the P V operand is two 8-byte reads;
// the head's table column (961 / 1521 floats) and, for SA, the 256 region ids.  Rows of keys outside the image are staged as zeros.
// 42000 bytes (SA) / 89296 bytes (OCA) per workgroup: three / one workgroup per CU.
//
// MFMA plan (v_mfma_f32_32x32x16), as in k_win_attn: the logits are produced TRANSPOSED, X = K Q^T (rows = keys, columns = queries), so a
// lane holds one query with 16 of the keys of a 32-key tile - key 32 kt + (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) - and a row reduction
// is the lane's own registers plus one lane ^ 32 exchange.  The rounded P^T tile is the A operand of the second product without any lane
// movement; its B operand is v[key][d = lane & 31] from the transposed LDS copy.  Q fragments come straight from global memory.
// Registers (bf16 build): SA 122 VGPRs + 24 AGPRs, OCA 135 VGPRs + 16 AGPRs, no scratch (3 waves per SIMD by registers).
//
// k_chan_pool1 / k_chan_pool2 - mean over H W per (sample, channel) in fp32: 64-row chunks (8 interleaved row subsets summed in order,
// then the subsets in order), then the chunks in order.  No atomics; the order depends on H W alone, not on B or the grid.
// k_chan_gate - per sample, fp32: s = scale * sigmoid(W2 relu(W1 pool + b1) + b2).   k_scale_add - y += c2 * s[b], one fma, one rounding,
// 16-byte accesses.   k_pixel_shuffle2 - 64 input bytes -> four 16-byte stores, bit copies.
#include "kernels.h"
#include "../../include/gyre_hip.h"
#include <algorithm>
#include <atomic>
#include <cmath>

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

namespace {
struct HatAttnParams {
    const bf16_t* qkv; int ld_qkv;
    bf16_t* o; int ld_o;
    const float* table;           // [961 | 1521][heads]
    int B, H, W, heads, shift;
};

template <bool OCA> struct HatGeom {
    static constexpr int NK = OCA ? 576 : 256;                    // keys per window
    static constexpr int NT = OCA ? 1521 : 961;                   // table rows
    static constexpr int KP = 40;                                 // K row pitch, elements
    static constexpr int VP = NK + 4;                             // V^T row pitch, elements
    static constexpr size_t K_BYTES = (size_t)NK * KP * 2;
    static constexpr size_t V_BYTES = (size_t)32 * VP * 2;
    static constexpr size_t T_BYTES = ((size_t)NT * 4 + 15) / 16 * 16;
    static constexpr size_t ID_BYTES = OCA ? 0 : 1024;
    static constexpr size_t LDS = K_BYTES + V_BYTES + T_BYTES + ID_BYTES;
};

__device__ __forceinline__ int hat_region(int Y, int L, int s) { return Y < L - 16 ? 0 : (Y < L - s ? 1 : 2); }

template <bool OCA>
__global__ __launch_bounds__(256) void k_hat_attn(HatAttnParams p) {
    using G = HatGeom<OCA>;
    extern __shared__ __attribute__((aligned(16))) unsigned char hat_smem[];
    bf16_t* Ks = (bf16_t*)hat_smem;
    bf16_t* Vt = (bf16_t*)(hat_smem + G::K_BYTES);
    float* tbl = (float*)(hat_smem + G::K_BYTES + G::V_BYTES);
    int* ids = (int*)(hat_smem + G::K_BYTES + G::V_BYTES + G::T_BYTES);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nwx = p.W >> 4, nwy = p.H >> 4;
    unsigned rest = blockIdx.x;
    const int head = (int)(rest % (unsigned)p.heads); rest /= (unsigned)p.heads;
    const int wx = (int)(rest % (unsigned)nwx); rest /= (unsigned)nwx;
    const int wy = (int)(rest % (unsigned)nwy);
    const int b = (int)(rest / (unsigned)nwy);
    const int s = OCA ? 0 : p.shift;
    const size_t img0 = (size_t)b * p.H * p.W;
    // query / SA key token t (0 .. 255) of this window -> row of the token-order tensors
    auto tok_row = [&](int t) -> size_t {
        int y = 16 * wy + (t >> 4) + s; if (y >= p.H) y -= p.H;
        int x = 16 * wx + (t & 15) + s; if (x >= p.W) x -= p.W;
        return img0 + (size_t)y * p.W + x;
    };

    // ---- stage K, V^T, the table column and the region ids
    const bf16_t* kb = p.qkv + 32 * (p.heads + head);
    const bf16_t* vb = p.qkv + 32 * (2 * p.heads + head);
    for (int idx = tid; idx < G::NK * 4; idx += 256) {
        const int slot = idx >> 2, piece = idx & 3;
        bool in = true;
        size_t row;
        if (OCA) {
            const int ey = slot / 24, ex = slot - 24 * ey;
            const int y = 16 * wy - 4 + ey, x = 16 * wx - 4 + ex;
            in = y >= 0 && y < p.H && x >= 0 && x < p.W;
            row = in ? img0 + (size_t)y * p.W + x : 0;
        } else {
            row = tok_row(slot);
        }
        uint4 k4 = {0u, 0u, 0u, 0u}, v4 = {0u, 0u, 0u, 0u};
        if (in) {
            k4 = *(const uint4*)(kb + row * p.ld_qkv + 8 * piece);
            v4 = *(const uint4*)(vb + row * p.ld_qkv + 8 * piece);
        }
        *(uint4*)(Ks + slot * G::KP + 8 * piece) = k4;
        const uint32_t w[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) Vt[(8 * piece + e) * G::VP + slot] = (bf16_t)(w[e >> 1] >> (16 * (e & 1)));
    }
    for (int idx = tid; idx < G::NT; idx += 256) tbl[idx] = p.table[(size_t)idx * p.heads + head];
    if (!OCA) ids[tid] = s ? 3 * hat_region(16 * wy + (tid >> 4), p.H, s) + hat_region(16 * wx + (tid & 15), p.W, s) : 0;
    __syncthreads();

    const int r = lane & 31, hh = lane >> 5;
    const float scale = 0.18257418583505536f;            // 30^-1/2
    const bf16_t* qb = p.qkv + 32 * head;

#pragma unroll 1
    for (int qt = 0; qt < 2; ++qt) {
        const int qtok = 64 * wave + 32 * qt + r;
        const int qi = qtok >> 4, qj = qtok & 15;
        const bf16_t* qp = qb + tok_row(qtok) * p.ld_qkv + 8 * hh;
        const bf16x8_t q0 = *(const bf16x8_t*)(qp), q1 = *(const bf16x8_t*)(qp + 16);
        const int qid = OCA ? 0 : ids[qtok];
        // bias index = qbase + (key term): SA (qi - ki + 15) 31 + (qj - kj + 15); OCA (ey - qi - 7) 39 + (ex - qj - 7), wrapped below
        const int qbase = OCA ? (-qi - 7) * 39 - qj - 7 : (qi + 15) * 31 + qj + 15;
        // the 32 x 32 logit tile kt: register 4 g + i of this lane is key 32 kt + 8 g + 4 hh + i against query qtok
        auto logits = [&](int kt) -> f32x16_t {
            const bf16_t* kr = Ks + (32 * kt + r) * G::KP + 8 * hh;
            const bf16x8_t k0 = *(const bf16x8_t*)(kr), k1 = *(const bf16x8_t*)(kr + 16);
            f32x16_t acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            acc = GYRE_MFMA_32x32x16(k0, q0, acc, 0, 0, 0);
            acc = GYRE_MFMA_32x32x16(k1, q1, acc, 0, 0, 0);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int key0 = 32 * kt + 8 * g + 4 * hh;          // four consecutive keys of one key row (16 and 24 are multiples of 4)
                int idx0;
                if (OCA) {
                    const int ey = key0 / 24, ex0 = key0 - 24 * ey;
                    idx0 = qbase + ey * 39 + ex0;
                } else {
                    idx0 = qbase - ((key0 >> 4) * 31 + (key0 & 15));
                }
                int kid[4] = {0, 0, 0, 0};
                if (!OCA && s) {
                    const int4 k4 = *(const int4*)(ids + key0);
                    kid[0] = k4.x; kid[1] = k4.y; kid[2] = k4.z; kid[3] = k4.w;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    int idx = OCA ? idx0 + i : idx0 - i;
                    if (OCA && idx < 0) idx += 1521;
                    float l = fmaf(scale, acc[4 * g + i], tbl[idx]);
                    if (!OCA && s && kid[i] != qid) l += -100.f;
                    acc[4 * g + i] = l;
                }
            }
            return acc;
        };

        // ---- pass 1: row maximum and row sum
        float m = -3.0e38f, sum = 0.f;
#pragma unroll 1
        for (int kt = 0; kt < G::NK / 32; ++kt) {
            const f32x16_t x = logits(kt);
            float tm = x[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) tm = fmaxf(tm, x[i]);
            const float mn = fmaxf(m, tm);
            float ts = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) ts += __expf(x[i] - mn);
            sum = fmaf(sum, __expf(m - mn), ts);
            m = mn;
        }
        const float mo = __shfl_xor(m, 32, 64), so = __shfl_xor(sum, 32, 64);
        const float M = fmaxf(m, mo);
        const float total = sum * __expf(m - M) + so * __expf(mo - M);       // the same two products in both lanes of the query
        const float inv = 1.0f / total;

        // ---- pass 2: P = exp(l - M) / S rounded to storage, O = P V
        f32x16_t oacc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int kt = 0; kt < G::NK / 32; ++kt) {
            f32x16_t x = logits(kt);
#pragma unroll
            for (int i = 0; i < 16; ++i) x[i] = __expf(x[i] - M) * inv;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                uint4 u;
                u.x = pack_bf16x2(x[8 * t + 0], x[8 * t + 1]);
                u.y = pack_bf16x2(x[8 * t + 2], x[8 * t + 3]);
                u.z = pack_bf16x2(x[8 * t + 4], x[8 * t + 5]);
                u.w = pack_bf16x2(x[8 * t + 6], x[8 * t + 7]);
                // element j of this lane: v[key 32 kt + 16 t + 8 (j >> 2) + 4 hh + (j & 3)][d = r]
                const bf16_t* vp = Vt + r * G::VP + 32 * kt + 16 * t + 4 * hh;
                const uint2 lo = *(const uint2*)(vp), hi = *(const uint2*)(vp + 8);
                const uint4 vv = {lo.x, lo.y, hi.x, hi.y};
                oacc = GYRE_MFMA_32x32x16(__builtin_bit_cast(bf16x8_t, u), __builtin_bit_cast(bf16x8_t, vv), oacc, 0, 0, 0);
            }
        }
        // tile [query 64 wave + 32 qt + (reg & 3) + 8 (reg >> 2) + 4 hh][d = r]
        if (r < 30) {
            bf16_t* ob = p.o + 30 * head + r;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int tq = 64 * wave + 32 * qt + (i & 3) + 8 * (i >> 2) + 4 * hh;
                ob[tok_row(tq) * p.ld_o] = f32_to_bf16(oacc[i]);
            }
        }
    }
}

// ---- channel attention ------------------------------------------------------------------------------------------------------
// block (chunk, b): rows [64 chunk, 64 chunk + 64) of sample b; thread (sub = t / 32, grp = t % 32) sums rows sub, sub + 8, ... of the
// chunk for the channels [8 grp, 8 grp + 8); then thread c adds the 8 subsets in order
__global__ __launch_bounds__(256) void k_chan_pool1(const bf16_t* __restrict__ x, int ld, size_t HW, int C, int nchunk, float* __restrict__ partial) {
    __shared__ float red[8][256];
    const int chunk = blockIdx.x, b = blockIdx.y;
    const int grp = threadIdx.x & 31, sub = threadIdx.x >> 5;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (8 * grp < C) {
        const size_t r0 = (size_t)chunk * 64;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const size_t row = r0 + sub + 8 * k;
            if (row < HW) {
                float f[8];
                unpack8(*(const uint4*)(x + ((size_t)b * HW + row) * ld + 8 * grp), f);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += f[j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) red[sub][8 * grp + j] = acc[j];
    __syncthreads();
    const int c = threadIdx.x;
    if (c < C) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) t += red[k][c];
        partial[((size_t)b * nchunk + chunk) * C + c] = t;
    }
}
__global__ __launch_bounds__(256) void k_chan_pool2(const float* __restrict__ partial, int nchunk, int C, float hw, float* __restrict__ pool) {
    const int b = blockIdx.x, c = threadIdx.x;
    if (c >= C) return;
    float t = 0.f;
    for (int k = 0; k < nchunk; ++k) t += partial[((size_t)b * nchunk + k) * C + c];
    pool[(size_t)b * C + c] = t / hw;
}
__global__ __launch_bounds__(256) void k_chan_gate(const float* __restrict__ pool, int C, int Cs, const float* __restrict__ w1,
                                                   const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                   float scale, float* __restrict__ s, int ld_s) {
    __shared__ float h[8];
    const int b = blockIdx.x, t = threadIdx.x;
    if (t < Cs) {
        float a = b1[t];
        for (int c = 0; c < C; ++c) a = fmaf(w1[(size_t)t * C + c], pool[(size_t)b * C + c], a);
        h[t] = a <= 0.f ? 0.f : a;                     // keeps a NaN, as torch's relu does (fmaxf would return 0)
    }
    __syncthreads();
    for (int c = t; c < ld_s; c += 256) {
        float v = 0.f;
        if (c < C) {
            float z = b2[c];
            for (int j = 0; j < Cs; ++j) z = fmaf(w2[(size_t)c * Cs + j], h[j], z);
            v = scale * (1.0f / (1.0f + expf(-z)));
        }
        s[(size_t)b * ld_s + c] = v;
    }
}
__global__ void k_scale_add(bf16_t* __restrict__ y, int ldy, const bf16_t* __restrict__ c2, int ldc, const float* __restrict__ s, int ld_s,
                            size_t HW, int G, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int g = (int)(i % (size_t)G);
    const size_t row = i / (size_t)G, b = row / HW;
    float yv[8], cv[8];
    bf16_t* yp = y + row * ldy + 8 * g;
    unpack8(*(const uint4*)yp, yv);
    unpack8(*(const uint4*)(c2 + row * ldc + 8 * g), cv);
    const float4 s0 = *(const float4*)(s + b * ld_s + 8 * g), s1 = *(const float4*)(s + b * ld_s + 8 * g + 4);
    const float sv[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) yv[j] = fmaf(cv[j], sv[j], yv[j]);
    *(uint4*)yp = pack8(yv);
}
// thread (pixel, g): input channels [32 g, 32 g + 32) -> output channels [8 g, 8 g + 8) of the four pixels (2 y + i, 2 x + j)
__global__ void k_pixel_shuffle2(const bf16_t* __restrict__ x, int ld_x, int H, int W, int G, bf16_t* __restrict__ out, int ld_out, size_t total) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int g = (int)(idx % (size_t)G);
    const size_t pix = idx / (size_t)G;
    const int xx = (int)(pix % (size_t)W);
    const size_t by = pix / (size_t)W;                      // b * H + y
    const size_t bb = by / (size_t)H, yy = by % (size_t)H;
    const uint4* src = (const uint4*)(x + pix * ld_x + 32 * g);
    uint32_t w[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint4 v = src[k];
        w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
    }
#pragma unroll
    for (int ij = 0; ij < 4; ++ij) {
        uint32_t o[4];
#pragma unroll
        for (int k2 = 0; k2 < 4; ++k2) {
            const int n0 = 4 * (2 * k2) + ij, n1 = 4 * (2 * k2 + 1) + ij;       // input channels 32 g + 4 c + 2 i + j for c = 2 k2, 2 k2 + 1
            const uint32_t e0 = (w[n0 >> 1] >> (16 * (n0 & 1))) & 0xffffu, e1 = (w[n1 >> 1] >> (16 * (n1 & 1))) & 0xffffu;
            o[k2] = e0 | (e1 << 16);
        }
        const size_t orow = ((bb * 2 * H + 2 * yy + (ij >> 1)) * 2 * W + 2 * xx + (ij & 1));
        const uint4 ov = {o[0], o[1], o[2], o[3]};
        *(uint4*)(out + orow * ld_out + 8 * g) = ov;
    }
}
}  // namespace

int hat_attn_check(const bf16_t* qkv, int ld_qkv, const bf16_t* o, int ld_o, const float* table, int mode, int B, int H, int W, int heads,
                   int shift) {
    if (!qkv || !o || !table) GYRE_FAIL(GYRE_ERR_INVALID, "hat_attn: null argument");
    if (mode != HAT_ATTN_SA && mode != HAT_ATTN_OCA) GYRE_FAIL(GYRE_ERR_INVALID, "hat_attn: mode 0 (self-attention) or 1 (overlapping cross-attention)");
    if (B < 1 || H < 16 || W < 16 || H % 16 || W % 16) GYRE_FAIL(GYRE_ERR_INVALID, "hat_attn: H and W must be positive multiples of the window size 16");
    if (heads < 1 || heads > 8) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "hat_attn: 1 to 8 heads of 30 channels are built");
    if (shift != 0 && shift != 8) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "hat_attn: the shift is 0 or half the window (8)");
    if (mode == HAT_ATTN_OCA && shift) GYRE_FAIL(GYRE_ERR_INVALID, "hat_attn: the overlapping cross-attention is not shifted");
    if (ld_qkv < 96 * heads || ld_o < 30 * heads) GYRE_FAIL(GYRE_ERR_INVALID, "hat_attn: row strides below 96 heads (qkv) / 30 heads (o)");
    if (ld_qkv % 8 || ((size_t)qkv & 15) || ((size_t)table & 3) || ((size_t)o & 1))
        GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "hat_attn: qkv needs 16-byte aligned rows (stride a multiple of 8)");
    if ((size_t)B * (H / 16) * (W / 16) * heads >= (1ull << 31)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "hat_attn: grid limits");
    return 0;
}
int launch_hat_attn(hipStream_t st, const bf16_t* qkv, int ld_qkv, bf16_t* o, int ld_o, const float* table, int mode, int B, int H, int W,
                    int heads, int shift) {
    int rc = hat_attn_check(qkv, ld_qkv, o, ld_o, table, mode, B, H, W, heads, shift);
    if (rc) return rc;
    HatAttnParams p;
    p.qkv = qkv; p.ld_qkv = ld_qkv; p.o = o; p.ld_o = ld_o; p.table = table; p.B = B; p.H = H; p.W = W; p.heads = heads; p.shift = shift;
    const unsigned blocks = (unsigned)((size_t)B * (H / 16) * (W / 16) * heads);
    const double nk = mode == HAT_ATTN_OCA ? 576.0 : 256.0;
    // Q K^T twice and P V once, 32 stored columns each; q, o and the staged k, v rows
    GyreProfScope prof(KC_ATTN, st, blocks * 3.0 * 2.0 * 256 * nk * 32, blocks * (2.0 * nk * 64 + 256 * 64 + 256 * 60));
    if (mode == HAT_ATTN_OCA) {
        auto kern = k_hat_attn<true>;
        static std::atomic<unsigned long long> attr_done{0};
        if (gyre_lds_attr_needed(attr_done))
            (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)HatGeom<true>::LDS);
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), HatGeom<true>::LDS, st, p);
    } else {
        hipLaunchKernelGGL(k_hat_attn<false>, dim3(blocks), dim3(256), HatGeom<false>::LDS, st, p);
    }
    GYRE_LAUNCH_CHECK();
    return 0;
}

size_t chan_pool_partial_floats(int B, size_t HW, int C) {
    if (B < 1 || HW < 1 || C < 1) return 0;
    return (size_t)B * ((HW + 63) / 64) * (size_t)C;
}
int launch_chan_pool(hipStream_t st, const bf16_t* x, int ld, int B, size_t HW, int C, float* partial, float* pool) {
    if (!x || !partial || !pool) GYRE_FAIL(GYRE_ERR_INVALID, "chan_pool: null argument");
    if (B < 1 || HW < 1 || C < 1) GYRE_FAIL(GYRE_ERR_INVALID, "chan_pool: bad sizes");
    if (C > 256) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "chan_pool: at most 256 channels");
    if (ld < (C + 7) / 8 * 8) GYRE_FAIL(GYRE_ERR_INVALID, "chan_pool: the row stride must cover the channels rounded up to 8");
    if (ld % 8 || ((size_t)x & 15)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "chan_pool: 16-byte aligned rows (stride a multiple of 8)");
    const size_t nchunk = (HW + 63) / 64;
    if (B > 65535 || nchunk >= (1ull << 31)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "chan_pool: grid limits");
    GyreProfScope prof(KC_OTHER, st, (double)B * HW * C, 2.0 * B * HW * C);
    hipLaunchKernelGGL(k_chan_pool1, dim3((unsigned)nchunk, (unsigned)B), dim3(256), 0, st, x, ld, HW, C, (int)nchunk, partial);
    GYRE_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_chan_pool2, dim3((unsigned)B), dim3(256), 0, st, (const float*)partial, (int)nchunk, C, (float)HW, pool);
    GYRE_LAUNCH_CHECK();
    return 0;
}
int launch_chan_gate(hipStream_t st, const float* pool, int B, int C, int Cs, const float* w1, const float* b1, const float* w2,
                     const float* b2, float scale, float* s, int ld_s) {
    if (!pool || !w1 || !b1 || !w2 || !b2 || !s) GYRE_FAIL(GYRE_ERR_INVALID, "chan_gate: null argument");
    if (B < 1 || C < 1 || Cs < 1 || ld_s < C) GYRE_FAIL(GYRE_ERR_INVALID, "chan_gate: bad sizes");
    if (C > 256 || Cs > 8) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "chan_gate: at most 256 channels squeezed to at most 8");
    hipLaunchKernelGGL(k_chan_gate, dim3((unsigned)B), dim3(256), 0, st, pool, C, Cs, w1, b1, w2, b2, scale, s, ld_s);
    GYRE_LAUNCH_CHECK();
    return 0;
}
int launch_scale_add(hipStream_t st, bf16_t* y, int ldy, const bf16_t* c2, int ldc, const float* s, int ld_s, int B, size_t HW, int Cn) {
    if (!y || !c2 || !s) GYRE_FAIL(GYRE_ERR_INVALID, "scale_add: null argument");
    if (B < 1 || HW < 1 || Cn < 8 || ldy < Cn || ldc < Cn || ld_s < Cn) GYRE_FAIL(GYRE_ERR_INVALID, "scale_add: the strides must cover the channels");
    if (Cn % 8 || ldy % 8 || ldc % 8 || ld_s % 4 || (((size_t)y | (size_t)c2 | (size_t)s) & 15))
        GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "scale_add: channels in multiples of 8 on 16-byte aligned rows");
    const size_t total = (size_t)B * HW * (Cn / 8);
    if (total >= (1ull << 31) * 256) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "scale_add: grid limits");
    GyreProfScope prof(KC_OTHER, st, 2.0 * B * HW * Cn, 6.0 * B * HW * Cn);
    hipLaunchKernelGGL(k_scale_add, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, y, ldy, c2, ldc, s, ld_s, HW, Cn / 8, total);
    GYRE_LAUNCH_CHECK();
    return 0;
}
int launch_pixel_shuffle2(hipStream_t st, const bf16_t* x, int ld_x, int B, int H, int W, int Co, bf16_t* out, int ld_out) {
    if (!x || !out) GYRE_FAIL(GYRE_ERR_INVALID, "pixel_shuffle2: null argument");
    if (B < 1 || H < 1 || W < 1 || Co < 8 || ld_x < 4 * Co || ld_out < Co) GYRE_FAIL(GYRE_ERR_INVALID, "pixel_shuffle2: the strides must cover 4 Co / Co channels");
    if (Co % 8 || ld_x % 8 || ld_out % 8 || (((size_t)x | (size_t)out) & 15))
        GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "pixel_shuffle2: output channels in multiples of 8 on 16-byte aligned rows");
    const size_t total = (size_t)B * H * W * (Co / 8);
    if (total >= (1ull << 31) * 256) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "pixel_shuffle2: grid limits");
    GyreProfScope prof(KC_OTHER, st, 0.0, 16.0 * B * H * W * Co);
    hipLaunchKernelGGL(k_pixel_shuffle2, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, ld_x, H, W, Co / 8, out, ld_out, total);
    GYRE_LAUNCH_CHECK();
    return 0;
}
