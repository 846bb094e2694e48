// Fused delta-merge repack (gfx950): k_repack_conv / k_repack_linear (kernels_elem.hip) with a sum of adapter TERMS - LoRA pairs and
// the LyCORIS forms - folded in front of the single rounding to the storage type, plus the small core contraction that turns a
// Tucker form into an operand of such a term.
//
//   out[o][ky][kx][ci] = round_storage( scale_p * ( base[so, ci, ky, kx] + sum_j s_j * D_j[so, ci, ky, kx] ) )
//
// base and every operand in PyTorch layout (base OIHW or [O][I]), each fp32, bf16 or fp16 on its own (load_as_f32: exact
// conversions).  so = o, or geglu_src_row(o) for the 16-row value / gate interleave of the GEGLU projection: every operand row
// follows the SOURCE row.  Pad columns (ci >= I) are written as +0.  t = ky KW + kx is the tap, KK = KH KW.
//
// A PRODUCT P(up [R][r], down [r][C][KK]; row, col, t) is  p = 0;  for q = 0 .. r - 1 ascending:  p = fma(up[row, q], down[q, col, t], p).
// Term kinds (D in fp32):
//   LORA   d = P(up0, down0; so, ci, t)                                              up0 [O][r], down0 [r][I][KK]
//   HADA   d1 = P(up0, down0; so, ci, t);  d2 = P(up1, down1; so, ci, t);  d = d1 * d2     each pair its own rank and dtype
//   KRON   d2 = P(up0 [O2][r], down0 [r][I2][KK]; so % O2, ci % I2, t)   or, rank0 == 0,  d2 = dense[so % O2, ci % I2, t]  (down0)
//          d = w1[so / O2][ci / I2] * d2                                             w1 dense fp32 [O1][I1], O = O1 O2, I = I1 I2
//   FULL   d = diff[so, ci, t]                                                       (down0)
//
// Operation order (fp32, restated by the host emulations in tests/lora_ref.py and tests/lyco_ref.py - change all or none):
//   acc = base
//   for j in argument order:  d = D_j as above (HADA: d1 completely, then d2, then one multiplication)
//                             acc = fma(s_j, d, acc)
//   out = round_storage(acc * scale_p)                      one multiplication after the sum, as k_repack_conv applies Param::scale
// With no terms this is k_repack_conv (and k_repack_linear where scale_p = 1) bit for bit.
//
// Form: one 256-thread workgroup per 64 x 64 tile of (output row) x (repacked column c = t I_pad + ci); each lane owns a 4 x 4 fp32
// tile (rows 4 ty .., columns 4 tx ..: the 4 columns are K-contiguous, one 8-byte store per row).  The two operands of a product
// pass through LDS in rank chunks of 32 (the last one partial), converted to fp32 while staged, so every factor element is read
// from memory once per tile instead of once per output element; a HADA term stages its second product through the same two buffers
// after the first.  A 64-row tile and a lane's 4 columns may both straddle a Kronecker factor boundary (O2 = 24, I2 = 6 ...): the
// staging computes row % O2 and col % I2 per staged element and the w1 factor is looked up per output element, nothing is assumed
// per tile or per lane.
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
//   All of this is REASONED from the banking rules; no LDS counter was collected for this kernel.  MEASURED are only the
//   request times in profiles/lora_request_time.json, profiles/lyco_request_time.json and profiles/adapter_path_refactor.json.
// 2 x 32 x 68 x 4 = 17 KB of LDS.  A HADA term holds d1, d2 and acc (48 accumulator registers), and with every kind inlined the
// compiler reports 141 VGPRs, no scratch, 3 waves per SIMD - three resident workgroups per CU, whose staging phases overlap each
// other's FMA phases.  The dense forms (KRON dense right factor, FULL) read their operand once per output element, like base.
// So the tile has a compile-time LORA_ONLY flag that takes kind = DELTA_LORA as a constant and never reads da.kind: the other kinds'
// code and registers are gone, the fma chain on the same values is the same.  launch_repack_delta picks that instantiation of
// k_repack_delta exactly when every term is a LORA term (a LoRA file, a LoCon with or without a mid tensor; no terms at all) - from
// the arguments, there is no switch.  That instantiation has 68 VGPRs, no scratch, 7 waves per SIMD in both storage builds: occupancy
// is not its limiter, the fp32 FMA rate is (gyre_amd/build.py records both instantiations, tests/test_merge_delta_ref_host.py reads
// the record).
//
// k_merge_delta<OUT>: the same tile with another store policy (lyco_tile<OUT, false>), for a weight that lives outside the native store - a
// CLIP text encoder's nn.Linear, a plain row-major [O][I] tensor of the dtype the encoder was loaded in:
//   out[o][i] = round_out( base[o][i] + sum_j s_j * D_j[o][i] )        OUT = GYRE_F32 | GYRE_BF16 | GYRE_F16, in BOTH storage builds
// Matrix only (KK = 1), no interleave, no pad columns (I % 4 == 0), no scale_p.  Operation order (restated in
// tests/merge_delta_ref.py - change both or neither): exactly the one above up to and including the last fma; then
//   out = round_out(acc)      fp32: acc as it stands, 16 bytes per lane;  bf16 / fp16: (__bf16) / (_Float16) conversion, round to
//                             nearest even, 8 bytes per lane - explicit conversions, f32_to_bf16 means the BUILD's storage type
// With no terms and out type = base type this copies base bit for bit (exact conversion to fp32 and back): how an adapter is taken
// off.  out may overlap neither base nor an operand (other workgroups still read them): launch_merge_delta refuses that, as it
// refuses everything delta_args_check refuses, before the launch.  The three instantiations have KK, Ipad and geglu as constants:
// the compiler reports 117 VGPRs, no scratch, 4 waves per SIMD, 17 KB of LDS for each in both builds (gyre_amd/build.py records it,
// tests/test_merge_delta_ref_host.py reads the record); k_repack_delta, the packed instantiation of the same tile, keeps the numbers
// stated above.  These are the COMPILER's numbers; the LDS banking statements above are reasoned and hold for both kernels (same
// staging, same reads); MEASURED is only the request time in profiles/text_adapter_request_time.json.
//
// k_lyco_core:  out[a][c][t] = sum_b core[a][b][t] * right[b][c]   (fp32 out, b ascending with fma from 0, inputs of any dtype).
// down' = core(mid, down) makes a LoCon Tucker form a LORA term, wb' = core(t, wb) a LoHa / LoKr one; with T = 1 it is
// w1 = w1a @ w1b.  Runs once per uploaded file, one thread per output element.
#include "kernels.h"

#define LYCO_TILE 64
#define LYCO_RCHUNK 32
#define LYCO_LD 68

__device__ __forceinline__ int lyco_src_row(int r, int F, int geglu) { return geglu ? geglu_src_row(r, F) : r; }

// k_repack_conv's last step, f32_to_bf16(v * scale), kept as a function of its own: in the fp16 build the compiler contracts the
// scalar product and its conversion into one mixed-precision instruction (v_fma_mixlo_f16: ONE rounding), while four products
// side by side become v_pk_mul_f32 + v_cvt_pk_f16_f32 (rounded to fp32 first), which differs from set_weight's bits in about one
// element in 10^4.  Those bits are the contract (zero terms must restore them), so the expression is compiled in isolation here
// exactly as k_repack_conv has it; tests/test_gpu_lora_native.py compares every key of a model on both builds.
static __device__ __attribute__((noinline)) uint32_t lyco_scale_round(float v, float scale) { return f32_to_bf16(v * scale); }

// d += P(up, down) over this tile.  KRON: the pair is a Kronecker right factor, up row = src_row(o) % Omod, down column = ci % Imod
// of a [rank][Imod][KK] tensor; else (LORA, HADA) Omod = O and Imod = I, the remainders are the values themselves and are not taken.
template <bool KRON>
__device__ __forceinline__ void lyco_product(float (&d)[4][4], float (*Us)[LYCO_LD], float (*Ds)[LYCO_LD], const void* __restrict__ up,
                                             const void* __restrict__ down, int dt, int rank, int Omod, int Imod, int O, int I, int KK,
                                             int Ipad, int Kp, int F, int geglu, int row0, int col0, int tid, int tx, int ty) {
    for (int r0 = 0; r0 < rank; r0 += LYCO_RCHUNK) {
        const int nr = min(LYCO_RCHUNK, rank - r0);
        __syncthreads();                      // the previous chunk has been consumed
        for (int idx = tid; idx < LYCO_TILE * LYCO_RCHUNK; idx += 256) {
            const int rr = idx & (LYCO_RCHUNK - 1), m = idx / LYCO_RCHUNK;
            const int o = row0 + m;
            float v = 0.f;
            if (o < O && rr < nr) {
                const int so = lyco_src_row(o, F, geglu);
                v = load_as_f32(up, dt, (size_t)(KRON ? so % Omod : so) * rank + r0 + rr);
            }
            Us[rr][m] = v;
        }
        for (int idx = tid; idx < LYCO_TILE * LYCO_RCHUNK; idx += 256) {
            const int cc = idx & (LYCO_TILE - 1), rr = idx / LYCO_TILE;
            const int c = col0 + cc;
            float v = 0.f;
            if (c < Kp && rr < nr) {
                const int t = c / Ipad, ci = c % Ipad;
                if (ci < I) v = load_as_f32(down, dt, ((size_t)(r0 + rr) * Imod + (KRON ? ci % Imod : ci)) * KK + t);
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
}

// The tile of both kernels.  OUT is the store policy: LYCO_OUT_PACKED writes the repacked storage layout (k_repack_delta: tap-major
// padded columns, GEGLU interleave, round_storage(acc * scale_p)), GYRE_F32 / BF16 / F16 write a row-major [O][I] matrix of that type
// (k_merge_delta: KK = 1, Ipad = I, geglu = 0 are constants there, acc is rounded as it stands).  Everything in front of the store
// is the same code.  LORA_ONLY: every term is a LORA term (the launcher has looked), the kind is a constant and da.kind is not read.
#define LYCO_OUT_PACKED (-1)
template <int OUT, bool LORA_ONLY>
__device__ __forceinline__ void lyco_tile(const void* __restrict__ base, int bdt, int O, int I, int KK, int Ipad, int geglu, float scale_p,
                                          const DeltaArgs& da, void* __restrict__ outv) {
    if constexpr (OUT != LYCO_OUT_PACKED) { KK = 1; Ipad = I; geglu = 0; }
    __shared__ __attribute__((aligned(16))) float Us[LYCO_RCHUNK][LYCO_LD];
    __shared__ __attribute__((aligned(16))) float Ds[LYCO_RCHUNK][LYCO_LD];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int row0 = blockIdx.y * LYCO_TILE, col0 = blockIdx.x * LYCO_TILE;
    const int Kp = KK * Ipad, F = O / 2;

    // this lane's 4 rows (source rows) and 4 columns (tap, input channel)
    int srow[4];
    bool rok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int o = row0 + ty * 4 + i;
        rok[i] = o < O;
        srow[i] = rok[i] ? lyco_src_row(o, F, geglu) : 0;
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

    for (int p = 0; p < da.n; ++p) {            // (uniform over the workgroup: the barriers inside lyco_product are reached by all)
        const int kind = LORA_ONLY ? DELTA_LORA : da.kind[p];
        float d[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) d[i][j] = 0.f;
        if (kind == DELTA_LORA || kind == DELTA_HADA) {
            lyco_product<false>(d, Us, Ds, da.up[p][0], da.down[p][0], da.dtype[p][0], da.rank[p][0], O, I, O, I, KK, Ipad, Kp, F, geglu,
                         row0, col0, tid, tx, ty);
            if (kind == DELTA_HADA) {
                float e[4][4];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) e[i][j] = 0.f;
                lyco_product<false>(e, Us, Ds, da.up[p][1], da.down[p][1], da.dtype[p][1], da.rank[p][1], O, I, O, I, KK, Ipad, Kp, F, geglu,
                             row0, col0, tid, tx, ty);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) d[i][j] = d[i][j] * e[i][j];
            }
        } else if (kind == DELTA_KRON) {
            const int O2 = O / da.O1[p], I2 = I / da.I1[p], I1 = da.I1[p];
            if (da.rank[p][0] > 0) {
                lyco_product<true>(d, Us, Ds, da.up[p][0], da.down[p][0], da.dtype[p][0], da.rank[p][0], O2, I2, O, I, KK, Ipad, Kp, F, geglu,
                             row0, col0, tid, tx, ty);
            } else {
                const void* __restrict__ w2 = da.down[p][0];
                const int dt = da.dtype[p][0];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int ci = ci0 + j;
                        if (rok[i] && cok && ci < I) d[i][j] = load_as_f32(w2, dt, ((size_t)(srow[i] % O2) * I2 + ci % I2) * KK + tap);
                    }
            }
            const float* __restrict__ w1 = da.w1[p];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {     // per ELEMENT: the lane's 4 columns may lie in two column factors
                    const int ci = ci0 + j;
                    const float f = (rok[i] && cok && ci < I) ? w1[(size_t)(srow[i] / O2) * I1 + ci / I2] : 0.f;
                    d[i][j] = f * d[i][j];
                }
        } else {                                  // DELTA_FULL
            const void* __restrict__ df = da.down[p][0];
            const int dt = da.dtype[p][0];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ci = ci0 + j;
                    if (rok[i] && cok && ci < I) d[i][j] = load_as_f32(df, dt, ((size_t)srow[i] * I + ci) * KK + tap);
                }
        }
        const float s = da.s[p];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(s, d[i][j], acc[i][j]);
    }

    if (!cok) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (!rok[i]) continue;
        const size_t at = (size_t)(row0 + ty * 4 + i) * Kp + c0;
        if constexpr (OUT == 0) {                 // fp32: stored as computed, 16 bytes per lane (Kp = I, I % 4 == 0: all 4 columns valid)
            f32x4_t w = {acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
            *(f32x4_t*)((float*)outv + at) = w;
        } else {
            uint32_t h[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (OUT == LYCO_OUT_PACKED) h[j] = lyco_scale_round(ci0 + j < I ? acc[i][j] : 0.f, scale_p);
                else if constexpr (OUT == 1) h[j] = __builtin_bit_cast(uint16_t, (__bf16)acc[i][j]);          // round to nearest even, whatever
                else h[j] = __builtin_bit_cast(uint16_t, (_Float16)acc[i][j]);                                 // the library's storage type
            }
            uint2 w;
            w.x = h[0] | (h[1] << 16); w.y = h[2] | (h[3] << 16);
            *(uint2*)((uint16_t*)outv + at) = w;                                // 8 bytes per lane along K
        }
    }
}

template <bool LORA_ONLY>
__global__ __launch_bounds__(256) void k_repack_delta(const void* __restrict__ base, int bdt, int O, int I, int KK, int Ipad, int geglu,
                                                      float scale_p, DeltaArgs da, bf16_t* __restrict__ out) {
    lyco_tile<LYCO_OUT_PACKED, LORA_ONLY>(base, bdt, O, I, KK, Ipad, geglu, scale_p, da, out);
}

template <int OUT>
__global__ __launch_bounds__(256) void k_merge_delta(const void* __restrict__ base, int bdt, int O, int I, DeltaArgs da, void* __restrict__ out) {
    lyco_tile<OUT, false>(base, bdt, O, I, 1, I, 0, 1.f, da, out);
}

__global__ __launch_bounds__(256) void k_lyco_core(const void* __restrict__ core, int cdt, const void* __restrict__ right, int rdt,
                                                   int A, int B, int Cn, int T, float* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)A * Cn * T) return;
    const int t = (int)(idx % T), c = (int)(idx / T % Cn), a = (int)(idx / T / Cn);
    float v = 0.f;
    for (int b = 0; b < B; ++b)                   // b ascending
        v = fmaf(load_as_f32(core, cdt, ((size_t)a * B + b) * T + t), load_as_f32(right, rdt, (size_t)b * Cn + c), v);
    out[idx] = v;
}

// Every check is made here, before the launch: the kernel trusts these shapes.
int delta_args_check(const DeltaArgs& da, int O, int I, double KK, double* flops) {
    if (da.n < 0 || da.n > GYRE_DELTA_MAX_TERMS) GYRE_FAIL(-1, "repack_delta: 0 to 8 terms per call");
    double fl = 0;
    for (int p = 0; p < da.n; ++p) {
        const int kind = da.kind[p];
        if (kind < DELTA_LORA || kind > DELTA_FULL) GYRE_FAIL(-1, "repack_delta: unknown term kind");
        const int pairs = kind == DELTA_HADA ? 2 : 1;
        for (int q = 0; q < pairs; ++q) {
            if (da.dtype[p][q] < 0 || da.dtype[p][q] > 2) GYRE_FAIL(-1, "repack_delta: bad operand dtype");
            if (!da.down[p][q]) GYRE_FAIL(-1, "repack_delta: null operand");
            const bool dense = kind == DELTA_FULL || (kind == DELTA_KRON && da.rank[p][q] == 0);
            if (dense) continue;
            if (!da.up[p][q]) GYRE_FAIL(-1, "repack_delta: null operand");
            if (da.rank[p][q] < 1) GYRE_FAIL(-1, "repack_delta: rank must be >= 1");
        }
        if (kind == DELTA_KRON) {
            if (!da.w1[p]) GYRE_FAIL(-1, "repack_delta: null operand (w1 of a Kronecker term)");
            if (da.rank[p][0] < 0) GYRE_FAIL(-1, "repack_delta: rank must be >= 1, or 0 for a dense right factor");
            if (da.O1[p] < 1 || da.I1[p] < 1 || O % da.O1[p] || I % da.I1[p])
                GYRE_FAIL(-1, "repack_delta: the Kronecker factor sizes do not multiply to the weight's (O1 must divide O, I1 must divide I)");
            fl += 2.0 * O * I * KK * da.rank[p][0];
        } else if (kind != DELTA_FULL) {
            fl += 2.0 * O * I * KK * (da.rank[p][0] + (kind == DELTA_HADA ? da.rank[p][1] : 0));
        }
    }
    if (flops) *flops = fl;
    return 0;
}

int launch_repack_delta(hipStream_t st, const void* base, int base_dtype, int O, int I, int KH, int KW, int Ipad, int geglu,
                        float scale_p, const DeltaArgs& da, bf16_t* out) {
    if (O < 1 || I < 1 || KH < 1 || KW < 1 || Ipad < I || Ipad % 4) GYRE_FAIL(-1, "repack_delta: needs O, I, KH, KW >= 1 and I_pad >= I, a multiple of 4");
    if (base_dtype < 0 || base_dtype > 2) GYRE_FAIL(-1, "repack_delta: bad base dtype");
    if (geglu && (O % 32 || KH != 1 || KW != 1)) GYRE_FAIL(-1, "repack_delta: the geglu interleave needs a matrix with O % 32 == 0");
    double flops = 0;
    if (int rc = delta_args_check(da, O, I, (double)KH * KW, &flops)) return rc;
    if ((size_t)O * KH * KW * Ipad >= ((size_t)1 << 31)) GYRE_FAIL(-1, "repack_delta: matrix too large");
    const int Kp = KH * KW * Ipad;
    GyreProfScope prof_(KC_LORA, st, flops, (double)O * Kp * 2.0 + (double)O * I * KH * KW * (base_dtype == 0 ? 4.0 : 2.0));
    bool lora_only = true;                        // (no terms: the plain repack, which needs no kind either)
    for (int p = 0; p < da.n; ++p) lora_only = lora_only && da.kind[p] == DELTA_LORA;
    const dim3 grid((Kp + LYCO_TILE - 1) / LYCO_TILE, (O + LYCO_TILE - 1) / LYCO_TILE);
    if (lora_only) hipLaunchKernelGGL(k_repack_delta<true>, grid, dim3(256), 0, st, base, base_dtype, O, I, KH * KW, Ipad, geglu, scale_p, da, out);
    else hipLaunchKernelGGL(k_repack_delta<false>, grid, dim3(256), 0, st, base, base_dtype, O, I, KH * KW, Ipad, geglu, scale_p, da, out);
    GYRE_LAUNCH_CHECK();
    return 0;
}

// [p, p + bytes) and [q, q + qbytes) share a byte
static inline bool lyco_overlap(const void* p, size_t bytes, const void* q, size_t qbytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qbytes && b < a + bytes;
}

int launch_merge_delta(hipStream_t st, const void* base, int base_dtype, int O, int I, const DeltaArgs& da, void* out, int out_dtype) {
    if (!base || !out) GYRE_FAIL(-1, "merge_delta: null argument");
    if (O < 1 || I < 1 || I % 4) GYRE_FAIL(-1, "merge_delta: needs O, I >= 1 and I a multiple of 4");
    if (base_dtype < 0 || base_dtype > 2 || out_dtype < 0 || out_dtype > 2) GYRE_FAIL(-1, "merge_delta: bad base or output dtype");
    double flops = 0;
    if (int rc = delta_args_check(da, O, I, 1.0, &flops)) return rc;
    if ((size_t)O * I >= ((size_t)1 << 31)) GYRE_FAIL(-1, "merge_delta: matrix too large");
    const size_t esz[3] = {4, 2, 2};
    const size_t n = (size_t)O * I, obytes = n * esz[out_dtype];
    if ((uintptr_t)out % (4 * esz[out_dtype])) GYRE_FAIL(-1, "merge_delta: out must be aligned to 4 elements");
    // the kernel reads base and the operands while other workgroups store: out may share no byte with any of them
    bool alias = lyco_overlap(out, obytes, base, n * esz[base_dtype]);
    for (int p = 0; p < da.n; ++p) {
        const int kind = da.kind[p];
        const size_t Ro = kind == DELTA_KRON ? (size_t)(O / da.O1[p]) : (size_t)O, Co = kind == DELTA_KRON ? (size_t)(I / da.I1[p]) : (size_t)I;
        for (int q = 0; q < (kind == DELTA_HADA ? 2 : 1); ++q) {
            const size_t e = esz[da.dtype[p][q]], r = (size_t)da.rank[p][q];
            const bool dense = kind == DELTA_FULL || (kind == DELTA_KRON && r == 0);
            alias |= lyco_overlap(out, obytes, da.down[p][q], (dense ? Ro : r) * Co * e);
            if (!dense) alias |= lyco_overlap(out, obytes, da.up[p][q], Ro * r * e);
        }
        if (kind == DELTA_KRON) alias |= lyco_overlap(out, obytes, da.w1[p], (size_t)da.O1[p] * da.I1[p] * 4);
    }
    if (alias) GYRE_FAIL(-1, "merge_delta: out overlaps base or an operand (the caller keeps the original weight)");
    GyreProfScope prof_(KC_LORA, st, flops, (double)obytes + (double)n * esz[base_dtype]);
    const dim3 grid((I + LYCO_TILE - 1) / LYCO_TILE, (O + LYCO_TILE - 1) / LYCO_TILE);
    if (out_dtype == 0) hipLaunchKernelGGL(k_merge_delta<0>, grid, dim3(256), 0, st, base, base_dtype, O, I, da, out);
    else if (out_dtype == 1) hipLaunchKernelGGL(k_merge_delta<1>, grid, dim3(256), 0, st, base, base_dtype, O, I, da, out);
    else hipLaunchKernelGGL(k_merge_delta<2>, grid, dim3(256), 0, st, base, base_dtype, O, I, da, out);
    GYRE_LAUNCH_CHECK();
    return 0;
}

int launch_lyco_core(hipStream_t st, const void* core, int core_dtype, const void* right, int right_dtype, int A, int B, int Cn, int T,
                     float* out) {
    if (!core || !right || !out) GYRE_FAIL(-1, "lyco_core: null argument");
    if (A < 1 || B < 1 || Cn < 1 || T < 1) GYRE_FAIL(-1, "lyco_core: needs A, B, C, T >= 1");
    if (core_dtype < 0 || core_dtype > 2 || right_dtype < 0 || right_dtype > 2) GYRE_FAIL(-1, "lyco_core: bad dtype");
    const size_t n = (size_t)A * Cn * T;
    if (n >= ((size_t)1 << 31)) GYRE_FAIL(-1, "lyco_core: output too large");
    GyreProfScope prof_(KC_LORA, st, 2.0 * n * B, 4.0 * n + 2.0 * ((double)A * B * T + (double)B * Cn));
    hipLaunchKernelGGL(k_lyco_core, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, core, core_dtype, right, right_dtype, A, B, Cn, T, out);
    GYRE_LAUNCH_CHECK();
    return 0;
}
