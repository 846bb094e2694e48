// Kernels of the token-sequence T2I networks (StyleAdapter, CoAdapterFuser: gyre/pipeline/t2i_adapter/adapter.py:135-343): multi-head
// self-attention over the packed in_proj output, QuickGELU, and the two ends of the co-adapter fuser (pooled feature, channel gain).
//
// k_seq_attn<D> - one 128-thread workgroup per (sample, head, block of 64 queries); wave w owns the 32 queries [64 qb + 32 w, + 32).
//
//   qkv [N L][ld_qkv]   the in_proj GEMM's output, sample-major rows (row n L + l); head h reads q at columns [h D, h D + D), k at
//                       W + h D, v at 2 W + h D, W = heads D.  Columns past 3 W and rows past N L are never read.
//   o   [N L][ld_o]     head h written at columns [h D, h D + D) of the rows n L + l, l < L; nothing else is written.
//
// Arithmetic, per query a over the L keys (no mask, no bias):
//   l[a][b] = scale * sum_d q[a][d] k[b][d]            fp32; scale = fl32(D^-1/2) applied to the fp32 dot product
//   p[a][b] = exp(l[a][b] - M[a]) / S[a]               fp32 statistics over the L real keys, rounded ONCE to storage
//   o[a][d] = sum_b p[a][b] v[b][d]                    fp32 accumulation, rounded once to storage
// The logits are computed twice, as in k_hat_attn (kernels_hat.hip): pass 1 keeps per lane a running maximum m and the sum of
// exp(l - m), rescaled when a 32-key tile raises the maximum, and merges the two lanes of a query; pass 2 recomputes the same logits
// (same instructions, same operands, same bits), forms p = exp(l - M) * (1 / S), rounds it and multiplies by V.
//
// LDS.  K and V of the (sample, head) are staged once: K rows [Lp][D + 8] storage (Lp = L rounded up to 32; the 16-byte pad keeps the
// fragment reads of 32 consecutive rows off one bank group), V TRANSPOSED [D][Lp + 4], written element-wise so that the P V operand is
// two 8-byte reads.  The slots [L, Lp) are staged as zeros and their logits are -inf: they take no part in the maximum, the sum or the
// product, whatever the memory behind them holds.  Lp (D + 8) 2 + D (Lp + 4) 2 bytes must fit the 160 KiB of a CU: L <= 1120 / 576 /
// 384 / 288 at D = 32 / 64 / 96 / 128 (seq_attn_max_len); beyond that, or for another D, the launcher refuses.
//
// MFMA plan (v_mfma_f32_32x32x16), as in k_hat_attn: the logits are produced TRANSPOSED, X = K Q^T (rows = keys, columns = queries), so a
// lane holds one query with 16 of the keys of a 32-key tile - key 32 kt + (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) - and a row reduction
// is the lane's own registers plus one lane ^ 32 exchange.  The rounded P^T tile is the A operand of the second product without any lane
// movement; its B operand is v[key][d = 32 dt + (lane & 31)] from the transposed LDS copy, one accumulator tile per 32 output columns.
// Q fragments come straight from global memory; queries past L are zeros and are not stored.
//
// k_quick_gelu  - x sigmoid(1.702 x) in place, fp32 (libm expf, IEEE division), one rounding.
// k_fuser_pool  - one wave per (sample, channel) of an NCHW map: lane i adds the elements i, i + 64, ... in order, the 64 partial sums
//                 are added by a fixed shuffle tree, mean = sum / (h w), out = silu(mean) rounded once to storage.  No atomics: the order
//                 depends on h w alone.
// k_fuser_gain  - out = x (alpha[n][c] + 1) or out += x (alpha[n][c] + 1) over an NCHW map; the sum alpha + 1, the product and the
//                 addition are separate fp32 roundings (no fma), then one rounding to storage.
// k_seq_rows    - the token passes of the two graphs: dst row = ((src row + add0) + add1 row) with every operand optional, between any
//                 two boundary dtypes - the concat with the broadcast style_embedding, + task_embedding[idx] (+ positional_embedding),
//                 and the gather of one sequence row per sample as fp32.
// k_seq_token_gain - out = tok (g + 1) on the style side (adapter.py:320), g the storage output of x @ seq_proj.
// k_repack_transposed - a parameter used as x @ P stored as P^T, the row-major form the GEMMs read (proj, seq_proj).
#include "kernels.h"
#include "../../include/gyre_hip.h"
#include <atomic>
#include <cmath>

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

namespace {
constexpr size_t SEQ_LDS_MAX = 160 * 1024;

struct SeqAttnParams {
    const bf16_t* qkv; int ld_qkv;
    bf16_t* o; int ld_o;
    int L, Lp, heads, qblocks;
    float scale;
};

inline size_t seq_attn_lds(int Lp, int D) { return (size_t)Lp * (D + 8) * 2 + (size_t)D * (Lp + 4) * 2; }

template <int D>
__global__ __launch_bounds__(128) void k_seq_attn(SeqAttnParams p) {
    constexpr int KP = D + 8;                   // K row pitch, elements
    constexpr int NS = D / 16;                  // K steps of the logit product
    constexpr int DT = D / 32;                  // 32-column tiles of the output
    constexpr int PC = D / 8;                   // 16-byte pieces of a row
    extern __shared__ __attribute__((aligned(16))) unsigned char seq_smem[];
    const int L = p.L, Lp = p.Lp, VP = Lp + 4;
    bf16_t* Ks = (bf16_t*)seq_smem;
    bf16_t* Vt = (bf16_t*)(seq_smem + (size_t)Lp * KP * 2);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned rest = blockIdx.x;
    const int qb = (int)(rest % (unsigned)p.qblocks); rest /= (unsigned)p.qblocks;
    const int head = (int)(rest % (unsigned)p.heads);
    const int n = (int)(rest / (unsigned)p.heads);
    const int W = p.heads * D;
    const size_t row0 = (size_t)n * L;

    // ---- stage K and V^T; the slots [L, Lp) are zeros
    const bf16_t* kb = p.qkv + W + head * D;
    const bf16_t* vb = p.qkv + 2 * W + head * D;
    for (int idx = tid; idx < Lp * PC; idx += 128) {
        const int slot = idx / PC, piece = idx - slot * PC;
        uint4 k4 = {0u, 0u, 0u, 0u}, v4 = {0u, 0u, 0u, 0u};
        if (slot < L) {
            k4 = *(const uint4*)(kb + (row0 + slot) * p.ld_qkv + 8 * piece);
            v4 = *(const uint4*)(vb + (row0 + slot) * p.ld_qkv + 8 * piece);
        }
        *(uint4*)(Ks + slot * KP + 8 * piece) = k4;
        const uint32_t w[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) Vt[(8 * piece + e) * VP + slot] = (bf16_t)(w[e >> 1] >> (16 * (e & 1)));
    }
    __syncthreads();

    const int r = lane & 31, hh = lane >> 5;
    const int q0 = 64 * qb + 32 * wave;                  // first query of this wave's tile
    if (q0 >= L) return;                                 // (after the only barrier)
    const int qtok = q0 + r;
    bf16x8_t q[NS];
    {
        const bf16_t* qp = p.qkv + head * D + (row0 + qtok) * p.ld_qkv + 8 * hh;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            uint4 u = {0u, 0u, 0u, 0u};
            if (qtok < L) u = *(const uint4*)(qp + 16 * s);
            q[s] = __builtin_bit_cast(bf16x8_t, u);
        }
    }
    const float scale = p.scale;
    const int nkt = Lp >> 5;
    // the 32 x 32 logit tile kt: register 4 g + i of this lane is key 32 kt + 8 g + 4 hh + i against query qtok
    auto logits = [&](int kt) -> f32x16_t {
        const bf16_t* kr = Ks + (32 * kt + r) * KP + 8 * hh;
        f32x16_t acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NS; ++s) acc = GYRE_MFMA_32x32x16(*(const bf16x8_t*)(kr + 16 * s), q[s], acc, 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int key = 32 * kt + 8 * g + 4 * hh + i;
                acc[4 * g + i] = key < L ? scale * acc[4 * g + i] : -INFINITY;
            }
        return acc;
    };

    // ---- pass 1: row maximum and row sum (m stays finite: exp(-inf - m) = 0 for the slots past L)
    float m = -3.0e38f, sum = 0.f;
#pragma unroll 1
    for (int kt = 0; kt < nkt; ++kt) {
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
    f32x16_t oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[dt][i] = 0.f;
#pragma unroll 1
    for (int kt = 0; kt < nkt; ++kt) {
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
            const bf16x8_t pf = __builtin_bit_cast(bf16x8_t, u);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                // element j of this lane: v[key 32 kt + 16 t + 8 (j >> 2) + 4 hh + (j & 3)][d = 32 dt + r]
                const bf16_t* vp = Vt + (32 * dt + r) * VP + 32 * kt + 16 * t + 4 * hh;
                const uint2 lo = *(const uint2*)(vp), hi = *(const uint2*)(vp + 8);
                const uint4 vv = {lo.x, lo.y, hi.x, hi.y};
                oacc[dt] = GYRE_MFMA_32x32x16(pf, __builtin_bit_cast(bf16x8_t, vv), oacc[dt], 0, 0, 0);
            }
        }
    }
    // tile dt: [query q0 + (reg & 3) + 8 (reg >> 2) + 4 hh][d = 32 dt + r]
    bf16_t* ob = p.o + head * D + r;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int tq = q0 + (i & 3) + 8 * (i >> 2) + 4 * hh;
        if (tq < L) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) ob[(row0 + tq) * p.ld_o + 32 * dt] = f32_to_bf16(oacc[dt][i]);
        }
    }
}

__global__ void k_quick_gelu(bf16_t* __restrict__ x, size_t n8) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    float f[8];
    unpack8(*(const uint4*)(x + 8 * i), f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = f[j] / (1.0f + expf(-1.702f * f[j]));
    *(uint4*)(x + 8 * i) = pack8(f);
}

// wave (n, c): x [N][C][HW] storage -> out[n][c] = silu(mean) storage
__global__ __launch_bounds__(256) void k_fuser_pool(const bf16_t* __restrict__ x, size_t NC, int C, size_t HW, bf16_t* __restrict__ out, int ld_out) {
    const size_t nc = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (nc >= NC) return;
    const bf16_t* xp = x + nc * HW;
    float acc = 0.f;
    for (size_t i = lane; i < HW; i += 64) acc += bf16_to_f32(xp[i]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_down(acc, d, 64);
    if (lane == 0) {
        const float mean = acc / (float)HW;
        out[(nc / C) * ld_out + (nc % C)] = f32_to_bf16(silu_f(mean));
    }
}

template <bool ACC>
__global__ void k_fuser_gain(const bf16_t* __restrict__ x, const float* __restrict__ alpha, int ld_a, int C, size_t HW, size_t total,
                             bf16_t* __restrict__ out) {
#pragma clang fp contract(off)                               // out + x g must not become one fma: the product rounds on its own
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t nc = i / HW;
    const float g = alpha[(nc / C) * ld_a + (nc % C)] + 1.0f;
    float v = bf16_to_f32(x[i]) * g;
    if (ACC) v = bf16_to_f32(out[i]) + v;
    out[i] = f32_to_bf16(v);
}

// thread (n, r, c): dst[n][r][c] = ((src[n][r][c] + add0[c]) + add1[r][c]), every operand optional, fp32, one rounding
__global__ void k_seq_rows(SeqRows a, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % (size_t)a.W);
    const size_t nr = i / (size_t)a.W;
    const int r = (int)(nr % (size_t)a.R);
    const size_t n = nr / (size_t)a.R;
    float v = a.src ? load_as_f32(a.src, a.src_dtype, n * a.src_ss + (size_t)r * a.src_rs + c) : 0.f;
    if (a.add0) v += a.add0[c];
    if (a.add1) v += a.add1[(size_t)r * a.W + c];
    store_from_f32(a.dst, a.dst_dtype, n * a.dst_ss + (size_t)r * a.dst_rs + c, v);
}

// thread (n, t, c): out[n][t][c] = tok[n][t][c] (g[n][t][c] + 1): the sum, then the product, each rounded in fp32; one rounding to out
__global__ void k_seq_token_gain(SeqTokenGain a, size_t total) {
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % (size_t)a.W);
    const size_t nt = i / (size_t)a.W;
    const int t = (int)(nt % (size_t)a.T);
    const size_t n = nt / (size_t)a.T;
    const float g = bf16_to_f32(a.g[n * a.g_ss + (size_t)t * a.W + c]) + 1.0f;
    store_from_f32(a.out, a.dtype, n * a.out_ss + (size_t)t * a.W + c, load_as_f32(a.tok, a.dtype, i) * g);
}

// thread (c, r): dst[c][r] = src[r][c] (dst rows of pitch i_pad; the padding keeps the zeros of the allocation)
__global__ void k_repack_transposed(const void* __restrict__ src, int dtype, int R, int Cc, int i_pad, bf16_t* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)R * Cc) return;
    const int r = (int)(i % (size_t)R), c = (int)(i / (size_t)R);
    dst[(size_t)c * i_pad + r] = f32_to_bf16(load_as_f32(src, dtype, (size_t)r * Cc + c));
}
}  // namespace

int launch_seq_rows(hipStream_t st, const SeqRows& a) {
    if (!a.dst || (!a.src && !a.add0 && !a.add1)) GYRE_FAIL(GYRE_ERR_INVALID, "seq_rows: null argument");
    if (a.N < 1 || a.R < 1 || a.W < 1) GYRE_FAIL(GYRE_ERR_INVALID, "seq_rows: bad sizes");
    if (a.src_dtype < 0 || a.src_dtype > 2 || a.dst_dtype < 0 || a.dst_dtype > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    const size_t total = (size_t)a.N * a.R * a.W;
    if ((total + 255) / 256 >= (1ull << 31)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "seq_rows: grid limits");
    hipLaunchKernelGGL(k_seq_rows, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a, total);
    GYRE_LAUNCH_CHECK();
    return 0;
}
int launch_seq_token_gain(hipStream_t st, const SeqTokenGain& a) {
    if (!a.tok || !a.g || !a.out) GYRE_FAIL(GYRE_ERR_INVALID, "seq_token_gain: null argument");
    if (a.N < 1 || a.T < 1 || a.W < 1) GYRE_FAIL(GYRE_ERR_INVALID, "seq_token_gain: bad sizes");
    if (a.dtype < 0 || a.dtype > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    const size_t total = (size_t)a.N * a.T * a.W;
    if ((total + 255) / 256 >= (1ull << 31)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "seq_token_gain: grid limits");
    hipLaunchKernelGGL(k_seq_token_gain, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a, total);
    GYRE_LAUNCH_CHECK();
    return 0;
}
int launch_repack_transposed(hipStream_t st, const void* src, int dtype, int R, int Cc, int i_pad, bf16_t* dst) {
    if (!src || !dst) GYRE_FAIL(GYRE_ERR_INVALID, "repack_transposed: null argument");
    if (dtype < 0 || dtype > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    if (R < 1 || Cc < 1 || i_pad < R) GYRE_FAIL(GYRE_ERR_INVALID, "repack_transposed: bad sizes");
    const size_t total = (size_t)R * Cc;
    hipLaunchKernelGGL(k_repack_transposed, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, dtype, R, Cc, i_pad, dst);
    GYRE_LAUNCH_CHECK();
    return 0;
}

int seq_attn_max_len(int D) {
    if (D != 32 && D != 64 && D != 96 && D != 128) return 0;
    int Lp = (int)((SEQ_LDS_MAX - 8 * (size_t)D) / (4 * (size_t)D + 16)) / 32 * 32;
    while (seq_attn_lds(Lp, D) > SEQ_LDS_MAX) Lp -= 32;
    return Lp;
}
int seq_attn_check(const bf16_t* qkv, int ld_qkv, const bf16_t* o, int ld_o, int N, int L, int heads, int D) {
    if (!qkv || !o) GYRE_FAIL(GYRE_ERR_INVALID, "seq_attn: null argument");
    if (N < 1 || L < 1 || heads < 1) GYRE_FAIL(GYRE_ERR_INVALID, "seq_attn: N, L and heads must be positive");
    if (D != 32 && D != 64 && D != 96 && D != 128) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "seq_attn: head dims 32, 64, 96 and 128 are built");
    if (heads > 1024) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "seq_attn: at most 1024 heads");
    if (L > seq_attn_max_len(D))
        GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "seq_attn: K and V of one head must fit the LDS: at most " + std::to_string(seq_attn_max_len(D)) +
                                            " tokens at head dim " + std::to_string(D));
    if (ld_qkv < 3 * heads * D || ld_o < heads * D) GYRE_FAIL(GYRE_ERR_INVALID, "seq_attn: row strides below 3 heads D (qkv) / heads D (o)");
    if (ld_qkv % 8 || ((size_t)qkv & 15) || ((size_t)o & 1))
        GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "seq_attn: qkv needs 16-byte aligned rows (stride a multiple of 8)");
    if ((size_t)N * heads * ((L + 63) / 64) >= (1ull << 31)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "seq_attn: grid limits");
    return 0;
}
int launch_seq_attn(hipStream_t st, const bf16_t* qkv, int ld_qkv, bf16_t* o, int ld_o, int N, int L, int heads, int D) {
    int rc = seq_attn_check(qkv, ld_qkv, o, ld_o, N, L, heads, D);
    if (rc) return rc;
    SeqAttnParams p;
    p.qkv = qkv; p.ld_qkv = ld_qkv; p.o = o; p.ld_o = ld_o; p.L = L; p.Lp = (L + 31) / 32 * 32; p.heads = heads; p.qblocks = (L + 63) / 64;
    p.scale = (float)(1.0 / std::sqrt((double)D));
    const size_t lds = seq_attn_lds(p.Lp, D);
    const unsigned blocks = (unsigned)((size_t)N * heads * p.qblocks);
    const void* kern = D == 32 ? (const void*)k_seq_attn<32> : D == 64 ? (const void*)k_seq_attn<64> : D == 96 ? (const void*)k_seq_attn<96>
                                                                                                                : (const void*)k_seq_attn<128>;
    static std::atomic<unsigned long long> attr_done[4];
    if (lds > 64 * 1024 && gyre_lds_attr_needed(attr_done[D / 32 - 1]))
        GYRE_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEQ_LDS_MAX));
    // Q K^T twice and P V once over the padded keys; q, o and the staged k, v rows
    GyreProfScope prof(KC_ATTN, st, blocks * 3.0 * 2.0 * 64 * p.Lp * D, blocks * (2.0 * L * D * 2 + 2.0 * 64 * D * 2));
    if (D == 32) hipLaunchKernelGGL(k_seq_attn<32>, dim3(blocks), dim3(128), lds, st, p);
    else if (D == 64) hipLaunchKernelGGL(k_seq_attn<64>, dim3(blocks), dim3(128), lds, st, p);
    else if (D == 96) hipLaunchKernelGGL(k_seq_attn<96>, dim3(blocks), dim3(128), lds, st, p);
    else hipLaunchKernelGGL(k_seq_attn<128>, dim3(blocks), dim3(128), lds, st, p);
    GYRE_LAUNCH_CHECK();
    return 0;
}

int launch_quick_gelu(hipStream_t st, bf16_t* x, size_t n) {
    if (!x) GYRE_FAIL(GYRE_ERR_INVALID, "quick_gelu: null argument");
    if (n < 8 || n % 8 || ((size_t)x & 15)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "quick_gelu: a 16-byte aligned buffer of a multiple of 8 elements");
    if (n / 8 >= (1ull << 31) * 256) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "quick_gelu: grid limits");
    GyreProfScope prof(KC_OTHER, st, (double)n, 4.0 * n);
    hipLaunchKernelGGL(k_quick_gelu, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, st, x, n / 8);
    GYRE_LAUNCH_CHECK();
    return 0;
}

int launch_fuser_pool(hipStream_t st, const bf16_t* x, int N, int C, size_t HW, bf16_t* out, int ld_out) {
    if (!x || !out) GYRE_FAIL(GYRE_ERR_INVALID, "fuser_pool: null argument");
    if (N < 1 || C < 1 || HW < 1 || ld_out < C) GYRE_FAIL(GYRE_ERR_INVALID, "fuser_pool: bad sizes, or an output stride below C");
    if (HW > (1ull << 24)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "fuser_pool: at most 2^24 pixels per map (the count is divided in fp32)");
    const size_t NC = (size_t)N * C;
    if ((NC + 3) / 4 >= (1ull << 31)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "fuser_pool: grid limits");
    GyreProfScope prof(KC_OTHER, st, (double)NC * HW, 2.0 * NC * HW);
    hipLaunchKernelGGL(k_fuser_pool, dim3((unsigned)((NC + 3) / 4)), dim3(256), 0, st, x, NC, C, HW, out, ld_out);
    GYRE_LAUNCH_CHECK();
    return 0;
}

int launch_fuser_gain(hipStream_t st, const bf16_t* x, const float* alpha, int ld_a, int N, int C, size_t HW, bf16_t* out, int accumulate) {
    if (!x || !alpha || !out) GYRE_FAIL(GYRE_ERR_INVALID, "fuser_gain: null argument");
    if (N < 1 || C < 1 || HW < 1 || ld_a < C) GYRE_FAIL(GYRE_ERR_INVALID, "fuser_gain: bad sizes, or an alpha stride below C");
    if (accumulate != 0 && accumulate != 1) GYRE_FAIL(GYRE_ERR_INVALID, "fuser_gain: accumulate is 0 (assign) or 1 (add to out)");
    const size_t total = (size_t)N * C * HW;
    if ((total + 255) / 256 >= (1ull << 31)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "fuser_gain: grid limits");
    GyreProfScope prof(KC_OTHER, st, 3.0 * total, (accumulate ? 6.0 : 4.0) * total);
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (accumulate) hipLaunchKernelGGL(k_fuser_gain<true>, dim3(blocks), dim3(256), 0, st, x, alpha, ld_a, C, HW, total, out);
    else hipLaunchKernelGGL(k_fuser_gain<false>, dim3(blocks), dim3(256), 0, st, x, alpha, ld_a, C, HW, total, out);
    GYRE_LAUNCH_CHECK();
    return 0;
}
