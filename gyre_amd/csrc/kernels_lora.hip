// Fused LoRA delta-merge repack (gfx950): k_repack_conv / k_repack_linear (kernels_elem.hip) with the low-rank sum folded in
// front of the single rounding to the storage type.
//
//   out[o][ky][kx][ci] = round_storage( scale_p * ( base[so, ci, ky, kx] + sum_j s_j * sum_r up_j[so, r] * down_j[r, ci, ky, kx] ) )
//
// base / up_j / down_j in PyTorch layout (base OIHW or [O][I], up [O][r] (x 1 x 1), down [r][I] (x KH x KW)), each fp32, bf16 or
// fp16 on its own (load_as_f32: exact conversions).  so = o, or geglu_src_row(o) for the 16-row value / gate interleave of the
// GEGLU projection: the up factor's row follows the SOURCE row.  Pad columns (ci >= I) are written as +0.
//
// Operation order (fp32, restated by the host emulation in tests/lora_ref.py - change both or neither):
//   acc = base
//   for j in argument order:  d = 0;  for r = 0 .. rank_j - 1 ascending:  d = fma(up_j[so, r], down_j[r, ...], d)
//                             acc = fma(s_j, d, acc)
//   out = round_storage(acc * scale_p)                      one multiplication after the sum, as k_repack_conv applies Param::scale
// With no pairs this is k_repack_conv (and k_repack_linear where scale_p = 1) bit for bit.
//
// Form: one 256-thread workgroup per 64 x 64 tile of (output row) x (repacked column c = (ky KW + kx) I_pad + ci); each lane owns
// a 4 x 4 fp32 tile (rows 4 ty .., columns 4 tx ..: the 4 columns are K-contiguous, one 8-byte store per row).  up / down pass
// through LDS in rank chunks of 32 (the last one partial), converted to fp32 while staged, so every factor element is read from
// memory once per tile instead of once per output element.
//   Us[rr][row]  (row stride 68 floats): a lane reads its 4 rows as one ds_read_b128; the wave's 4 (ty) addresses broadcast.
//                Staged with lanes along r (contiguous in memory): a 32-lane store group holds one row m and rr = 0..31, word
//                offset 68 rr + m, i.e. bank (4 rr + m) mod 32 for ds_write_b32 - 8 banks, 4 addresses each, which by the
//                banking rules costs about 2x on a store.  An estimate from those rules, not a measured counter; it concerns
//                8 stores per lane and chunk beside 512 FMAs.
//   Ds[rr][col]  (row stride 68 floats): a lane reads its 4 columns as one ds_read_b128, the 16 tx addresses of a lane group
//                cover 64 distinct banks.  Staged in COLUMN order (lanes along the repacked column): the stride-KH*KW walk of a
//                3x3 factor is on the global side, where the L2 serves it (a down factor is r x I x 9 elements, < 1 MB), and the
//                LDS stores are bank-consecutive - the LDS image needs no padding beyond the 16-byte row alignment (likewise
//                reasoned from the banking rules, not measured; the alternative is a source-order gather into a padded image).
// 2 x 32 x 68 x 4 = 17 KB of LDS and 68 VGPRs: occupancy is not the limiter, the fp32 FMA rate is.
#include "kernels.h"

#define LORA_TILE 64
#define LORA_RCHUNK 32
#define LORA_LD 68

__device__ __forceinline__ int lora_src_row(int r, int F, int geglu) {          // geglu_src_row of kernels_elem.hip
    if (!geglu) return r;
    const int p = r >> 5, i = r & 31;
    return i < 16 ? p * 16 + i : F + p * 16 + (i - 16);
}

// k_repack_conv's last step, f32_to_bf16(v * scale), kept as a function of its own: in the fp16 build the compiler contracts the
// scalar product and its conversion into one mixed-precision instruction (v_fma_mixlo_f16: ONE rounding), while four products
// side by side become v_pk_mul_f32 + v_cvt_pk_f16_f32 (rounded to fp32 first), which differs from set_weight's bits in about one
// element in 10^4.  Those bits are the contract (zero pairs must restore them), so the expression is compiled in isolation here
// exactly as k_repack_conv has it; tests/test_gpu_lora_native.py compares every key of a model on both builds.
static __device__ __attribute__((noinline)) uint32_t lora_scale_round(float v, float scale) { return f32_to_bf16(v * scale); }

__global__ __launch_bounds__(256) void k_repack_lora(const void* __restrict__ base, int bdt, int O, int I, int KK, int Ipad, int geglu,
                                                     float scale_p, LoraArgs la, bf16_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float Us[LORA_RCHUNK][LORA_LD];
    __shared__ __attribute__((aligned(16))) float Ds[LORA_RCHUNK][LORA_LD];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int row0 = blockIdx.y * LORA_TILE, col0 = blockIdx.x * LORA_TILE;
    const int Kp = KK * Ipad, F = O / 2;

    // this lane's 4 rows (source rows) and 4 columns (tap, input channel)
    int srow[4];
    bool rok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int o = row0 + ty * 4 + i;
        rok[i] = o < O;
        srow[i] = rok[i] ? lora_src_row(o, F, geglu) : 0;
    }
    const int c0 = col0 + tx * 4;               // Kp % 4 == 0 and Ipad % 4 == 0: the 4 columns share validity and tap
    const bool cok = c0 < Kp;
    const int tap = cok ? c0 / Ipad : 0, ci0 = cok ? c0 % Ipad : 0;

    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ci = ci0 + j;
            acc[i][j] = (rok[i] && cok && ci < I) ? load_as_f32(base, bdt, ((size_t)srow[i] * I + ci) * KK + tap) : 0.f;
        }

    for (int p = 0; p < la.n; ++p) {
        const void* __restrict__ up = la.up[p];
        const void* __restrict__ down = la.down[p];
        const int dt = la.dtype[p], rank = la.rank[p];
        float d[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) d[i][j] = 0.f;
        for (int r0 = 0; r0 < rank; r0 += LORA_RCHUNK) {
            const int nr = min(LORA_RCHUNK, rank - r0);
            __syncthreads();                      // the previous chunk has been consumed
            for (int idx = tid; idx < LORA_TILE * LORA_RCHUNK; idx += 256) {
                const int rr = idx & (LORA_RCHUNK - 1), m = idx / LORA_RCHUNK;
                const int o = row0 + m;
                float v = 0.f;
                if (o < O && rr < nr) v = load_as_f32(up, dt, (size_t)lora_src_row(o, F, geglu) * rank + r0 + rr);
                Us[rr][m] = v;
            }
            for (int idx = tid; idx < LORA_TILE * LORA_RCHUNK; idx += 256) {
                const int cc = idx & (LORA_TILE - 1), rr = idx / LORA_TILE;
                const int c = col0 + cc;
                float v = 0.f;
                if (c < Kp && rr < nr) {
                    const int t = c / Ipad, ci = c % Ipad;
                    if (ci < I) v = load_as_f32(down, dt, ((size_t)(r0 + rr) * I + ci) * KK + t);
                }
                Ds[rr][cc] = v;
            }
            __syncthreads();
            for (int rr = 0; rr < nr; ++rr) {     // r ascending
                const f32x4_t a = *(const f32x4_t*)&Us[rr][ty * 4];
                const f32x4_t b = *(const f32x4_t*)&Ds[rr][tx * 4];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) d[i][j] = fmaf(a[i], b[j], d[i][j]);
            }
        }
        const float s = la.s[p];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(s, d[i][j], acc[i][j]);
    }

    if (!cok) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (!rok[i]) continue;
        uint32_t h[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) h[j] = lora_scale_round(ci0 + j < I ? acc[i][j] : 0.f, scale_p);
        uint2 w;
        w.x = h[0] | (h[1] << 16); w.y = h[2] | (h[3] << 16);
        *(uint2*)(out + (size_t)(row0 + ty * 4 + i) * Kp + c0) = w;         // 8 bytes per lane along K
    }
}

int launch_repack_lora(hipStream_t st, const void* base, int base_dtype, int O, int I, int KH, int KW, int Ipad, int geglu,
                       float scale_p, const LoraArgs& la, bf16_t* out) {
    if (O < 1 || I < 1 || KH < 1 || KW < 1 || Ipad < I || Ipad % 4) GYRE_FAIL(-1, "repack_lora: needs O, I, KH, KW >= 1 and I_pad >= I, a multiple of 4");
    if (base_dtype < 0 || base_dtype > 2) GYRE_FAIL(-1, "repack_lora: bad base dtype");
    if (geglu && (O % 32 || KH != 1 || KW != 1)) GYRE_FAIL(-1, "repack_lora: the geglu interleave needs a matrix with O % 32 == 0");
    if (la.n < 0 || la.n > GYRE_LORA_MAX_PAIRS) GYRE_FAIL(-1, "repack_lora: 0 to 8 LoRA pairs per call");
    double flops = 0;
    for (int p = 0; p < la.n; ++p) {
        if (!la.up[p] || !la.down[p]) GYRE_FAIL(-1, "repack_lora: null factor");
        if (la.dtype[p] < 0 || la.dtype[p] > 2) GYRE_FAIL(-1, "repack_lora: bad factor dtype");
        if (la.rank[p] < 1) GYRE_FAIL(-1, "repack_lora: rank must be >= 1");
        flops += 2.0 * O * I * KH * KW * la.rank[p];
    }
    if ((size_t)O * KH * KW * Ipad >= ((size_t)1 << 31)) GYRE_FAIL(-1, "repack_lora: matrix too large");
    const int Kp = KH * KW * Ipad;
    GyreProfScope prof_(KC_LORA, st, flops, (double)O * Kp * 2.0 + (double)O * I * KH * KW * (base_dtype == 0 ? 4.0 : 2.0));
    hipLaunchKernelGGL(k_repack_lora, dim3((Kp + LORA_TILE - 1) / LORA_TILE, (O + LORA_TILE - 1) / LORA_TILE), dim3(256), 0, st,
                       base, base_dtype, O, I, KH * KW, Ipad, geglu, scale_p, la, out);
    GYRE_LAUNCH_CHECK();
    return 0;
}
