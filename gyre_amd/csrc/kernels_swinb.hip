// Swin-B backbone kernels (model_swinb.hip): shifted-window attention over 12 x 12 windows at head dim 32 on a zero-padded map, the patch
// embedding with its LayerNorm, and the patch-merging gather with its LayerNorm.
//
// k_win12_attn - one WAVE per (sample, window, head); a workgroup is four waves with consecutive (window, head) numbers, head fastest, so
// the four heads of a Swin-B stage-0 window (and four of the 8 / 16 / 32 of the later stages) share a workgroup, the token map of the
// window and its lines of the qkv rows in L2.  The 144 tokens of a window are addressed in place: token (i, j) of window (wy, wx) under
// shift s is the pixel (y, x) = ((12 wy + i + s) mod Hp, (12 wx + j + s) mod Wp) of the map padded to Hp x Wp, multiples of 12.  A pixel
// with y >= H or x >= W is a PADDED token: the reference pads norm1's output with zeros, so its q / k / v are the qkv bias (rounded to
// storage, what the projection of a zero row stores); it is an ordinary key, and as a query it is computed and dropped.  Neither the
// padded, the rolled nor the window-partitioned tensor of the reference (SwinTransformer.py:209-244) ever exists.
//
//   qkv [B H W][ld_qkv]   fused projection output in token order: q of head h at columns [32 h, 32 h + 32), k at 32 (heads + h), v at
//                         32 (2 heads + h) - nn.Linear's own order at head dim 32, no repack
//   o   [B H W][ld_o]     head h at columns [32 h, 32 h + 32); no other column is written, every real token is
//
// Arithmetic, per (window, head), query a and key b (a = 12 i + j):
//   l[a][b] = scale * sum_d q[a][d] k[b][d] + bias[h][a][b] + (s > 0 and id(a) != id(b) ? -100 : 0)    fp32; scale = 32^-1/2 on the fp32 dot
//   p[a][b] = exp(l[a][b] - max_b l[a][.]) / sum_b exp(..)     fp32 over the whole 144-wide row in registers; rounded ONCE to storage
//   o[a][d] = sum_b p[a][b] v[b][d]                           fp32 accumulation, rounded once to storage
// id = 3 r(12 wy + i, Hp) + r(12 wx + j, Wp), r(Y, L) = 0 if Y < L - 12, 1 if Y < L - s, else 2: BasicLayer.forward's img_mask on the PADDED
// map, computed from the window position; the shift is 6 whatever the map size, so a map of one window is masked too.
//
// MFMA plan (v_mfma_f32_16x16x32; operand lane (fr, fq) = (lane & 15, lane >> 4) holds row / column fr and k = 8 fq .. 8 fq + 7, the
// result lane rows 4 fq .. 4 fq + 3 of column fr).  144 = 9 x 16 and D = 32 is ONE k step, so there is no key padding:
//   X = K Q^T, 9 x 9 tiles.  A: k[key 16 kt + fr][8 fq ..], B: q[query 16 qt + fr][8 fq ..], both one 16-byte read of a qkv row.  A lane
//       ends up with ONE query (16 qt + fr) and the keys 16 kt + 4 fq + i in register i of tile kt: a softmax row is the lane's own 36
//       registers and those of lanes ^ 16, ^ 32 - two exchanges per reduction.
//   O^T = V^T P^T, 5 k steps x 2 tiles of 16 d.  Step t multiplies the key tiles 2 t and 2 t + 1: element j of the lane is key
//       16 (2 t) + 4 fq + j for j < 4 and key 16 (2 t + 1) + 4 fq + j - 4 above, which are exactly the registers the lane holds, so the
//       rounded P^T is the B operand without lane movement (step 4: tile 8 and zeros).  A is v[that key][16 dt + fr].  The result lane
//       holds d = 16 dt + 4 fq .. + 3 of its own query: one 8-byte store per tile.
// Registers and LDS.  The nine K fragments (36 registers) and the ten V fragments (40) of the (window, head) are loaded once and stay
// in registers over the nine query tiles.  V goes through LDS: the wave stages its 144 x 32 V rows (9 KB, row pitch 40 elements, 16-byte
// reads of global rows) in its own slab and gathers the transposed fragments from there with 2-byte LDS reads, 16 lanes on 32
// contiguous bytes and the four lane groups 80 words apart.  46 KB per workgroup, one barrier.
//
// The expanded bias (launch_win12_bias) is stored in the register order of X, [head][query tile][key tile][lane][i] fp32, one coalesced
// 16-byte load per tile.
//
// k_swinb_embed    - PatchEmbed: 4 x 4 / stride 4 convolution of the zero-padded NCHW image and patch_embed.norm, one wave per token at a
//                    time.  The weights sit in LDS as fp32 [48][C] (rounded to storage first: what a GEMM would read); lane k < 48 loads
//                    input (c, ky, kx) = (k / 16, (k / 4) & 3, k & 3), rounded to storage, and broadcasts it; lane l accumulates channels
//                    l, l + 64, .. in fp32, k ascending; the LayerNorm (two-pass, fp32) follows on the unrounded sums, one rounding.
// k_swinb_merge_ln - PatchMerging up to its Linear: one wave per output token gathers the 2 x 2 neighbourhood in the reference's order
//                    (even, even), (odd, even), (even, odd), (odd, odd) with zeros past an odd map's edge, normalises the 4 C values
//                    (two-pass, fp32, the zeros included, as the reference pads before the norm) and writes the row the reduction GEMM
//                    reads: the [.., 4 C] tensor is written once and read once.
#include "kernels.h"
#include "../../include/gyre_hip.h"
#include <algorithm>

namespace {
constexpr int W12_VP = 40;                    // V slab row pitch, elements

struct Win12Params {
    const bf16_t* qkv; int ld_qkv; const float* qkv_bias;
    bf16_t* o; int ld_o;
    const float* bias;            // [heads][144 * 144] in register order
    int B, H, W, nwy, nwx, heads, shift;
    unsigned total;               // B * nwy * nwx * heads waves
};

__device__ __forceinline__ int win12_region(int Y, int L, int s) { return Y < L - 12 ? 0 : (Y < L - s ? 1 : 2); }

__global__ __launch_bounds__(256) void k_win12_attn(Win12Params p) {
    __shared__ __attribute__((aligned(16))) bf16_t vslab[4][144 * W12_VP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned wv = blockIdx.x * 4u + wave;
    const bool live = wv < p.total;
    if (!live) wv = p.total - 1;                         // (the wave keeps the barrier company and stores nothing)
    const int head = (int)(wv % (unsigned)p.heads);
    unsigned rest = wv / (unsigned)p.heads;
    const int wx = (int)(rest % (unsigned)p.nwx); rest /= (unsigned)p.nwx;
    const int wy = (int)(rest % (unsigned)p.nwy);
    const int b = (int)(rest / (unsigned)p.nwy);
    const int s = p.shift, Hp = 12 * p.nwy, Wp = 12 * p.nwx;
    const int fr = lane & 15, fq = lane >> 4;
    const size_t img0 = (size_t)b * p.H * p.W;
    // token t (0 .. 143) of this window -> row of the token-order tensors, -1 for a padded token
    auto tok_row = [&](int t) -> long long {
        const int i = t / 12, j = t - 12 * i;
        int y = 12 * wy + i + s; if (y >= Hp) y -= Hp;
        int x = 12 * wx + j + s; if (x >= Wp) x -= Wp;
        return y < p.H && x < p.W ? (long long)(img0 + (size_t)y * p.W + x) : -1;
    };
    auto tok_id = [&](int t) -> int {
        const int i = t / 12, j = t - 12 * i;
        return 3 * win12_region(12 * wy + i, Hp, s) + win12_region(12 * wx + j, Wp, s);
    };
    // eight consecutive columns of a token's qkv row; a padded token's are the bias, rounded as the projection would store it
    auto piece = [&](long long row, int col) -> uint4 {
        if (row >= 0) return *(const uint4*)(p.qkv + (size_t)row * p.ld_qkv + col);
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = p.qkv_bias[col + e];
        return pack8(f);
    };
    const int qcol = 32 * head, kcol = 32 * (p.heads + head), vcol = 32 * (2 * p.heads + head);

    // ---- V rows -> this wave's slab; K fragments (A operand of X = K Q^T), one per key tile
    bf16_t* vs = vslab[wave];
#pragma unroll
    for (int it = 0; it < 9; ++it) {
        const int idx = lane + 64 * it, t = idx >> 2, pc = idx & 3;
        *(uint4*)(vs + t * W12_VP + 8 * pc) = piece(tok_row(t), vcol + 8 * pc);
    }
    bf16x8_t kf[9];
    unsigned kid[9];                                     // the ids of this lane's four keys per tile, 4 bits each
#pragma unroll
    for (int kt = 0; kt < 9; ++kt) {
        kf[kt] = __builtin_bit_cast(bf16x8_t, piece(tok_row(16 * kt + fr), kcol + 8 * fq));
        unsigned w = 0;
        if (s) {
#pragma unroll
            for (int i = 0; i < 4; ++i) w |= (unsigned)tok_id(16 * kt + 4 * fq + i) << (4 * i);
        }
        kid[kt] = w;
    }
    __syncthreads();
    // V fragments (A operand of O^T = V^T P^T): [k step][d tile], element j = v[key(t, j)][16 dt + fr]
    bf16x8_t vf[5][2];
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            uint32_t w[4];
#pragma unroll
            for (int jp = 0; jp < 4; ++jp) {
                const int kt = 2 * t + (jp >> 1), key0 = 16 * kt + 4 * fq + 2 * (jp & 1);
                uint32_t lo = 0, hi = 0;
                if (kt < 9) { lo = vs[key0 * W12_VP + 16 * dt + fr]; hi = vs[(key0 + 1) * W12_VP + 16 * dt + fr]; }
                w[jp] = lo | (hi << 16);
            }
            const uint4 u = {w[0], w[1], w[2], w[3]};
            vf[t][dt] = __builtin_bit_cast(bf16x8_t, u);
        }
    const float scale = 0.17677669529663687f;            // 32^-1/2
    const float4* bias4 = (const float4*)(p.bias + (size_t)head * (144 * 144));

#pragma unroll 1
    for (int qt = 0; qt < 9; ++qt) {
        const int qtok = 16 * qt + fr;
        const long long qrow = tok_row(qtok);
        const bf16x8_t qf = __builtin_bit_cast(bf16x8_t, piece(qrow, qcol + 8 * fq));
        const unsigned qid = s ? (unsigned)tok_id(qtok) : 0u;
        f32x4_t x[9];
        float m = -3.0e38f;
#pragma unroll
        for (int kt = 0; kt < 9; ++kt) {
            f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
            acc = GYRE_MFMA_16x16x32(kf[kt], qf, acc, 0, 0, 0);
            const float4 bv = bias4[(qt * 9 + kt) * 64 + lane];
            const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float l = fmaf(scale, acc[i], bb[i]);
                if (s && ((kid[kt] >> (4 * i)) & 15u) != qid) l += -100.f;
                acc[i] = l;
                m = fmaxf(m, l);
            }
            x[kt] = acc;
        }
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < 9; ++kt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float e = __expf(x[kt][i] - m);
                x[kt][i] = e;
                sum += e;
            }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.0f / sum;
        f32x4_t oacc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            uint4 u = {0u, 0u, 0u, 0u};
            u.x = pack_bf16x2(x[2 * t][0] * inv, x[2 * t][1] * inv);
            u.y = pack_bf16x2(x[2 * t][2] * inv, x[2 * t][3] * inv);
            if (t < 4) {
                u.z = pack_bf16x2(x[2 * t + 1][0] * inv, x[2 * t + 1][1] * inv);
                u.w = pack_bf16x2(x[2 * t + 1][2] * inv, x[2 * t + 1][3] * inv);
            }
            const bf16x8_t pf = __builtin_bit_cast(bf16x8_t, u);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) oacc[dt] = GYRE_MFMA_16x16x32(vf[t][dt], pf, oacc[dt], 0, 0, 0);
        }
        // tile dt: [d = 16 dt + 4 fq + i][query qtok]
        if (live && qrow >= 0) {
            bf16_t* ob = p.o + (size_t)qrow * p.ld_o + 32 * head + 4 * fq;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                uint2 v;
                v.x = pack_bf16x2(oacc[dt][0], oacc[dt][1]);
                v.y = pack_bf16x2(oacc[dt][2], oacc[dt][3]);
                *(uint2*)(ob + 16 * dt) = v;
            }
        }
    }
}

// table [529][heads] fp32 -> the kernel's register order (header): bias[h][a][b] = table[(i - i' + 11) * 23 + (j - j' + 11)][h]
__global__ void k_win12_bias(const float* __restrict__ table, int heads, float* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= heads * 144 * 144) return;
    const int i = idx & 3, lane = (idx >> 2) & 63, blk = idx >> 8;
    const int kt = blk % 9, qt = (blk / 9) % 9, h = blk / 81;
    const int a = 16 * qt + (lane & 15), b = 16 * kt + 4 * (lane >> 4) + i;
    const int di = a / 12 - b / 12 + 11, dj = a % 12 - b % 12 + 11;
    out[idx] = table[(di * 23 + dj) * heads + h];
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float round_store(float f) { return bf16_to_f32(f32_to_bf16(f)); }

// NI = channels per lane (C <= 64 NI)
template <int NI>
__global__ __launch_bounds__(256) void k_swinb_embed(const void* __restrict__ x, int dtype, int H, int W, int Ht, int Wt, int C, size_t tokens,
                                                     const float* __restrict__ w, const float* __restrict__ bias,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                     bf16_t* __restrict__ y) {
    extern __shared__ float embed_w[];                   // [48][C]
    for (int idx = threadIdx.x; idx < 48 * C; idx += 256) {
        const int k = idx / C, c = idx - k * C;
        embed_w[idx] = round_store(w[c * 48 + k]);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    float bs[NI], g[NI], bt[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int c = lane + 64 * i;
        bs[i] = c < C ? bias[c] : 0.f; g[i] = c < C ? gamma[c] : 0.f; bt[i] = c < C ? beta[c] : 0.f;
    }
    const int kc = lane >> 4, ky = (lane >> 2) & 3, kx = lane & 3;
    for (size_t tok = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); tok < tokens; tok += (size_t)gridDim.x * 4) {
        const int tx = (int)(tok % Wt);
        const size_t r = tok / Wt;
        const int ty = (int)(r % Ht);
        const size_t b = r / Ht;
        const int py = 4 * ty + ky, px = 4 * tx + kx;
        float pix = 0.f;
        if (lane < 48 && py < H && px < W) pix = round_store(load_as_f32(x, dtype, ((b * 3 + kc) * H + py) * (size_t)W + px));
        float acc[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) acc[i] = 0.f;
#pragma unroll
        for (int k = 0; k < 48; ++k) {
            const float pk = __shfl(pix, k, 64);
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int c = lane + 64 * i;
                if (c < C) acc[i] = fmaf(pk, embed_w[k * C + c], acc[i]);
            }
        }
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            acc[i] = lane + 64 * i < C ? acc[i] + bs[i] : 0.f;
            sum += acc[i];
        }
        const float mean = wave_sum(sum) / (float)C;
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const float d = lane + 64 * i < C ? acc[i] - mean : 0.f;
            sq = fmaf(d, d, sq);
        }
        const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)C + eps);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = lane + 64 * i;
            if (c < C) y[tok * C + c] = f32_to_bf16(fmaf((acc[i] - mean) * rstd, g[i], bt[i]));
        }
    }
}

// one wave per output token; lane l holds the 8-element chunks l, l + 64, l + 128, l + 192 of the 4 C row
__global__ __launch_bounds__(256) void k_swinb_merge_ln(const bf16_t* __restrict__ x, int H, int W, int Ho, int Wo, int C, size_t tokens,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                        bf16_t* __restrict__ y) {
    const size_t tok = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tok >= tokens) return;                           // (whole waves: no barrier follows)
    const int lane = threadIdx.x & 63, C4 = 4 * C, nch = C4 >> 3;
    const int ox = (int)(tok % Wo);
    const size_t r = tok / Wo;
    const int oy = (int)(r % Ho);
    const size_t b = r / Ho;
    float v[4][8];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ch = lane + 64 * i;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
        if (ch < nch) {
            const int e0 = 8 * ch, q = e0 / C, c = e0 - q * C;
            const int sy = 2 * oy + (q & 1), sx = 2 * ox + (q >> 1);
            if (sy < H && sx < W) unpack8(*(const uint4*)(x + ((b * H + sy) * (size_t)W + sx) * C + c), v[i]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += v[i][e];
    }
    const float mean = wave_sum(sum) / (float)C4;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (lane + 64 * i < nch) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = v[i][e] - mean;
                sq = fmaf(d, d, sq);
            }
        }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)C4 + eps);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ch = lane + 64 * i;
        if (ch < nch) {
            float o8[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) o8[e] = fmaf((v[i][e] - mean) * rstd, gamma[8 * ch + e], beta[8 * ch + e]);
            *(uint4*)(y + tok * C4 + 8 * ch) = pack8(o8);
        }
    }
}
}  // namespace

int win12_attn_check(const bf16_t* qkv, int ld_qkv, const float* qkv_bias, const bf16_t* o, int ld_o, const float* bias, int B, int H, int W,
                     int heads, int shift) {
    if (!qkv || !qkv_bias || !o || !bias) GYRE_FAIL(GYRE_ERR_INVALID, "win12_attn: null argument");
    if (B < 1 || H < 1 || W < 1) GYRE_FAIL(GYRE_ERR_INVALID, "win12_attn: empty map");
    if (heads < 1 || heads > 64) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "win12_attn: 1 to 64 heads of 32 channels are built");
    if (shift != 0 && shift != 6) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "win12_attn: the shift is 0 or half the window (6)");
    if (ld_qkv < 96 * heads || ld_o < 32 * heads) GYRE_FAIL(GYRE_ERR_INVALID, "win12_attn: row strides below 96 heads (qkv) / 32 heads (o)");
    if (ld_qkv % 8 || ld_o % 4 || ((size_t)qkv & 15) || ((size_t)bias & 15) || ((size_t)o & 7))
        GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "win12_attn: qkv needs 16-byte aligned rows, o 8-byte aligned rows and bias a 16-byte aligned start");
    if ((size_t)B * ((H + 11) / 12) * ((W + 11) / 12) * heads >= (1ull << 31)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "win12_attn: grid limits");
    return 0;
}
int launch_win12_attn(hipStream_t st, const bf16_t* qkv, int ld_qkv, const float* qkv_bias, bf16_t* o, int ld_o, const float* bias, int B,
                      int H, int W, int heads, int shift) {
    int rc = win12_attn_check(qkv, ld_qkv, qkv_bias, o, ld_o, bias, B, H, W, heads, shift);
    if (rc) return rc;
    Win12Params p;
    p.qkv = qkv; p.ld_qkv = ld_qkv; p.qkv_bias = qkv_bias; p.o = o; p.ld_o = ld_o; p.bias = bias;
    p.B = B; p.H = H; p.W = W; p.nwy = (H + 11) / 12; p.nwx = (W + 11) / 12; p.heads = heads; p.shift = shift;
    p.total = (unsigned)((size_t)B * p.nwy * p.nwx * heads);
    const double pairs = (double)p.total;
    GyreProfScope prof(KC_ATTN, st, pairs * 2.0 * 2.0 * 144 * 144 * 32, pairs * (4.0 * 144 * 144 + 4.0 * 144 * 64));
    hipLaunchKernelGGL(k_win12_attn, dim3((p.total + 3) / 4), dim3(256), 0, st, p);
    GYRE_LAUNCH_CHECK();
    return 0;
}
int launch_win12_bias(hipStream_t st, const float* table, int heads, float* out) {
    if (!table || !out) GYRE_FAIL(GYRE_ERR_INVALID, "win12_bias: null argument");
    if (heads < 1 || heads > 64) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "win12_bias: 1 to 64 heads");
    hipLaunchKernelGGL(k_win12_bias, dim3(heads * 81), dim3(256), 0, st, table, heads, out);
    GYRE_LAUNCH_CHECK();
    return 0;
}
int launch_swinb_embed(hipStream_t st, const void* x, int dtype, int B, int H, int W, int C, const float* w, const float* bias,
                       const float* gamma, const float* beta, float eps, bf16_t* y) {
    if (!x || !w || !bias || !gamma || !beta || !y) GYRE_FAIL(GYRE_ERR_INVALID, "swinb_embed: null argument");
    if (dtype < 0 || dtype > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    if (B < 1 || H < 1 || W < 1) GYRE_FAIL(GYRE_ERR_INVALID, "swinb_embed: empty image");
    if (C < 32 || C % 32 || C > 256) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swinb_embed: C must be a multiple of 32, at most 256");
    const int Ht = (H + 3) / 4, Wt = (W + 3) / 4;
    const size_t tokens = (size_t)B * Ht * Wt;
    const unsigned blocks = (unsigned)std::min<size_t>((tokens + 3) / 4, 2048);       // the weights are staged once per workgroup
    const size_t lds = (size_t)48 * C * 4;
    GyreProfScope prof(KC_OTHER, st, 2.0 * 48 * C * tokens, (double)tokens * (48 * 4 + 2 * C));
#define GYRE_EMBED(NI) hipLaunchKernelGGL(k_swinb_embed<NI>, dim3(blocks), dim3(256), lds, st, x, dtype, H, W, Ht, Wt, C, tokens, w, bias, gamma, beta, eps, y)
    if (C <= 64) GYRE_EMBED(1);
    else if (C <= 128) GYRE_EMBED(2);
    else GYRE_EMBED(4);
#undef GYRE_EMBED
    GYRE_LAUNCH_CHECK();
    return 0;
}
int launch_swinb_merge_ln(hipStream_t st, const bf16_t* x, int B, int H, int W, int C, const float* gamma, const float* beta, float eps,
                          bf16_t* y) {
    if (!x || !gamma || !beta || !y) GYRE_FAIL(GYRE_ERR_INVALID, "swinb_merge_ln: null argument");
    if (B < 1 || H < 1 || W < 1) GYRE_FAIL(GYRE_ERR_INVALID, "swinb_merge_ln: empty map");
    if (C < 8 || C % 8 || 4 * C > 2048) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swinb_merge_ln: C must be a multiple of 8 with 4 C <= 2048");
    if (((size_t)x | (size_t)y) & 15) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swinb_merge_ln: 16-byte alignment");
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const size_t tokens = (size_t)B * Ho * Wo;
    if ((tokens + 3) / 4 >= (1ull << 31)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swinb_merge_ln: grid limits");
    GyreProfScope prof(KC_LAYERNORM, st, 8.0 * 4 * C * tokens, 16.0 * C * tokens);
    hipLaunchKernelGGL(k_swinb_merge_ln, dim3((unsigned)((tokens + 3) / 4)), dim3(256), 0, st, x, H, W, Ho, Wo, C, tokens, gamma, beta, eps, y);
    GYRE_LAUNCH_CHECK();
    return 0;
}
