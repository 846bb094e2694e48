// Host-side launchers of the hand-written gfx950 kernels.  All enqueue on `st`
// and return 0 / negative gyre_status (message via gyre_last_error()).
#pragma once
#include "common.h"

// ---- layout / small ops (kernels_elem.hip) ----------------------------------
int launch_nchw_to_nhwc(hipStream_t st, const void* x, int dtype, int B, int C, int HW, int Cpad, bf16_t* y);
// y[b][p][c] = rnd(x[b][c][p] * mask[mask_B == 1 ? 0 : b][p]): the product in fp32 from the source dtype, one rounding to storage
int launch_nchw_to_nhwc_masked(hipStream_t st, const void* x, int dtype, int B, int C, int HW, int Cpad, const float* mask, int mask_B,
                               bf16_t* y);
int launch_add_nchw_into_nhwc(hipStream_t st, const void* r, int dtype, int B, int C, int HW, int Cpad, bf16_t* y);
int launch_ctx_to_bf16(hipStream_t st, const void* x, int dtype, size_t n, bf16_t* y);
// dst[o][0:inner] = dst[o][inner:2*inner] = src[o][0:inner] (bytes, multiples of 16), o < outer
int launch_dup_batch(hipStream_t st, const void* src, void* dst, size_t outer, size_t inner_bytes);
int launch_add_f32(hipStream_t st, float* y, const float* x, size_t n);
// A Transformer2D's proj_out composed with the FF2 in front of it (C % 64 == 0; Wp [C][C], W2 [C][4C] storage rows, b2 / bp [C] f32 or null):
//   Wc[n][0:4C] = sum_k Wp[n][k] W2[k][j]  (fp32, k ascending, one rounding to the storage type), Wc[n][4C:5C] = Wp[n][:]   (Wc [C][5C])
//   bc[n] = sum_k Wp[n][k] b2[k] + bp[n]   (fp32, k ascending)
int launch_compose_proj(hipStream_t st, const bf16_t* Wp, const bf16_t* W2, const float* b2, const float* bp, int C, bf16_t* Wc, float* bc);
// debug (GYRE_VERIFY_HINTS=1): flag |= 1 if t[b] != t[0] for some b, |= 2 if the two halves of x (bytes_per_half each) differ
int launch_verify_hints(hipStream_t st, const int64_t* t, int B, int check_t, const void* x, size_t bytes_per_half, int check_pairs, int* flag);
int launch_timestep_embedding(hipStream_t st, const int64_t* t, int B, int dim, int flip, float shift, float* out);
// out[b][n] = sum_k f(x[b][k]) * W[n][k] + bias[n]; x f32 [B][K], W bf16 [N][K], out f32 [B][ldo].  act_in_silu: f = SiLU,
// and for B > 4 x is OVERWRITTEN with SiLU(x) (its only use on the time-embedding path; B <= 4 applies it on load)
int launch_rowvec_linear(hipStream_t st, float* x, int B, int K, const bf16_t* W, const float* bias, int N,
                         int act_in_silu, float* out, int ldo);
// out[b] = Linear(timestep_embedding(t[b])) - one launch for B <= 4 (emb_scratch [B][dim] floats is used above that)
int launch_timestep_linear(hipStream_t st, const int64_t* t, int B, int dim, int flip, float shift, float* emb_scratch,
                           const bf16_t* W, const float* bias, int N, float* out, int ldo);

// GroupNorm over NHWC bf16, optional second source for the skip-concat case:
// channels [0,C1) come from x (pixel stride C1), [C1,C) from x2 (pixel stride C-C1).
struct GnParams {
    const bf16_t* x; const bf16_t* x2; int C1;
    int B, HW, C, G;
    const float* gamma; const float* beta; float eps; int silu;
    float* partial;      // [B][nchunks][G][2]
    float* scale_shift;  // [B][2][C]   (a = rstd*gamma, b = beta - mean*a)
    int nchunks;
    bf16_t* y;           // [B][HW][C]
    float* mean_rstd = nullptr;  // optional [B][G][2] (backward pass)
    // statistics left by the producers of x / x2 (GemmParams::colstat_out): [B][cs_chunks][C_src / cs_unit][2] per source.
    // When cs_x is set (and cs_x2 for a dual-source call) launch_groupnorm_stats is not needed: launch_groupnorm_apply
    // finishes the group statistics from them in its prologue (cs_unit divides C1, C - C1 and C / G).
    const float* cs_x = nullptr; int cs_x_chunks = 0;
    const float* cs_x2 = nullptr; int cs_x2_chunks = 0;
    int cs_unit = 0;
};
size_t gn_workspace_bytes(int B, int HW, int C, int G);
int gn_pick_chunks(int B, int HW, int C);
// 0 = off; n > 0: plan every split-K factor as if the batch held n samples (results then do not depend on B)
int gemm_set_batch_invariant(int canonical_samples);
int gemm_get_batch_invariant();
// everything thread-local the planner's choices depend on (tuning flags, forced config, batch-invariant size, packed-weight
// scratch) folded into one value: callers that memoise plans key on it.  The low 32 bits are the tuning switches below.
long gemm_planner_state();
// Tuning switches tested on the host (gyre_debug_gemm_ablation, include/gyre_hip.h; per calling thread).  Results stay valid.
enum : int {
    GEMM_DBG_NO_SM            = 0x20,        // bit 5: no small-problem kernel (config 32): small linear problems go to the 4-wave tiles
    GEMM_DBG_SM_NO_SPLITK     = 0x40,        // bit 6: the small-problem kernel does not take the long-K few-row problems from split K
    GEMM_DBG_NO_SC_FOLD       = 0x80,        // bit 7: the 1x1 shortcut stays its own launch instead of riding inside conv2
    GEMM_DBG_CONV_ZERO_PAGE   = 0x200,       // bit 9: conv zero padding from a zero page in the pipelined kernel
    GEMM_DBG_NO_4S            = 0x400,       // bit 10: no pipelined (32x32x16) tile configs
    GEMM_DBG_NO_LN_FOLD       = 0x800,       // bit 11: LayerNorm as a separate pass (no fold into the consuming GEMM)
    GEMM_DBG_NO_GN_FOLD       = 0x1000,      // bit 12: the Transformer2D GroupNorm keeps its apply pass (no fold into proj_in)
    GEMM_DBG_NO_XATTN         = 0x2000,      // bit 13: no fused cross-attention kernel: the three-launch chain
    GEMM_DBG_NO_GEGLU_4S      = 0x4000,      // bit 14: the GEGLU FF1 does not take the pipelined 256x320 tile
    GEMM_DBG_LN_STATS_PASS    = 0x8000,      // bit 15: folded LayerNorm takes its row statistics from a separate pass
    GEMM_DBG_GEGLU_NO_LN_FOLD = 0x10000,     // bit 16: the GEGLU FF1 keeps its separate LayerNorm
    GEMM_DBG_GN_STATS_PASS    = 0x20000,     // bit 17: GroupNorm keeps its own statistics pass (no producer column statistics)
    GEMM_DBG_NO_128x160       = 0x40000,     // bit 18: no 128x160 (config 8) and 256x128 (config 12) tiles
    GEMM_DBG_NO_CS_128x160    = 0x100000,    // bit 20: no statistics epilogue on the 128x160 tile
    GEMM_DBG_NO_AR            = 0x200000,    // bit 21: no A-resident kernel (config 30)
    GEMM_DBG_AR_ALL           = 0x400000,    // bit 22: A-resident kernel also for the C x C projections (N < 3 K)
    GEMM_DBG_NO_4S_128_TILES  = 0x800000,    // bit 23: no pipelined 256x320 tile for 3x3 convs whose grid of it has 128 - 159 workgroups
    GEMM_DBG_TWO_STAGE_LINEAR = 0x1000000,   // bit 24: the two-stage K loop in the 8-wave kernels' linear mode
    GEMM_DBG_DEEP_RING        = 0x2000000,   // bit 25: the deep ring at one workgroup per CU also where two 2-stage workgroups fit
    GEMM_DBG_NO_W_BLOCK       = 0x4000000,   // bit 26: row-major weights everywhere (no blocked weight copies)
    GEMM_DBG_TWO_STAGE_CONV   = 0x8000000,   // bit 27: the two-stage K loop for the 128x160 / 256x128 tiles' 3x3 convolutions
    GEMM_DBG_NO_POUT_FOLD     = 0x10000000,  // bit 28: a Transformer2D's proj_out stays its own launch instead of riding inside the last FF2
    GEMM_DBG_NO_UPS4          = 0x20000000,  // bit 29: the upsampler convs keep nine taps (no four-parity 2x2 form, GemmParams::ups4)
    GEMM_DBG_UPS4_ALL         = 0x40000000,  // bit 30: the four-parity form wherever the kernel supports it: config 24 whatever the tile count
};
int launch_groupnorm_stats(hipStream_t st, const GnParams& p);   // partial sums + finalize -> scale_shift
int launch_groupnorm_apply(hipStream_t st, const GnParams& p);   // y = act(a*x+b)
bool gn_use_small(int HW, int C, int C1, int G);                 // one-launch path for small feature maps
bool gn_accepts_colstats(const GnParams& p);                     // cs_unit / shapes fit the producer-statistics form of the apply
int launch_groupnorm_small(hipStream_t st, const GnParams& p);
// GroupNorm (affine only) folded into the Linear / 1x1 conv W[N][C] (+ bias) that consumes it: per sample b the scaled weights
// Wf[b][N][C] (bf16) and the bias row bf[b][N] (fp32); statistics from p.cs_x (producer column statistics) or p.partial
// (launch_groupnorm_stats).  Consumed by a GEMM with GemmParams::w_sample_stride = N * C and rowbias = bf.
int launch_gn_fold(hipStream_t st, const GnParams& p, const bf16_t* W, const float* bias, int N, bf16_t* Wf, float* bf);
int launch_layernorm(hipStream_t st, const bf16_t* x, int M, int C, const float* gamma, const float* beta, float eps,
                     bf16_t* y);
// stats[m] = (rstd, rstd * mean) of row m: the input of a GEMM with the LayerNorm folded in (GemmParams::ln_stats)
int launch_layernorm_stats(hipStream_t st, const bf16_t* x, int M, int C, float eps, float* stats);

// weight repack: OIHW (any dtype) -> [O][KH][KW][Ipad] bf16 ; linear [O][I] -> bf16 (optionally GEGLU-interleaved)
int launch_nhwc_to_nchw_f32(hipStream_t st, const bf16_t* x, int B, int C, int HW, int Cpad, float* y);
int launch_repack_conv(hipStream_t st, const void* w, int dtype, int O, int I, int KH, int KW, int Ipad, bf16_t* out,
                       float scale = 1.f);
int launch_repack_linear(hipStream_t st, const void* w, int dtype, int O, int I, int geglu_interleave, bf16_t* out);
int launch_cast_f32(hipStream_t st, const void* w, int dtype, size_t n, int geglu_interleave, float* out, float scale = 1.f);
int launch_copy_probe(hipStream_t st, const void* src, void* dst, size_t bytes);
// fused delta-merge repack (kernels_lyco.hip): launch_repack_conv / _linear of  base + sum_j s[j] D_j  (operands in PyTorch layout,
// each in its own dtype), summed in fp32 in front of the one rounding; n = 0 gives the plain repack's bits.  A TERM D_j is a
// low-rank product (LORA: a LoRA pair, up [O][rank], down [rank][I][KH][KW]), the Hadamard product of two (HADA), a Kronecker
// product of a dense w1 with a low-rank or dense right factor (KRON), or a dense diff (FULL).  LORA terms alone (or none) run a
// LoRA-only instantiation of the kernel, chosen from the arguments.  Operand layouts, the rank == 0 convention of a dense KRON right
// factor and the operation order: header of kernels_lyco.hip.  Kind values are those of gyre_delta_term (include/gyre_hip.h).
#define GYRE_DELTA_MAX_TERMS 8
enum { DELTA_LORA = 0, DELTA_HADA = 1, DELTA_KRON = 2, DELTA_FULL = 3 };
struct DeltaArgs {
    int kind[GYRE_DELTA_MAX_TERMS];
    const void* up[GYRE_DELTA_MAX_TERMS][2];
    const void* down[GYRE_DELTA_MAX_TERMS][2];
    int dtype[GYRE_DELTA_MAX_TERMS][2];
    int rank[GYRE_DELTA_MAX_TERMS][2];
    const float* w1[GYRE_DELTA_MAX_TERMS];
    int O1[GYRE_DELTA_MAX_TERMS], I1[GYRE_DELTA_MAX_TERMS];
    float s[GYRE_DELTA_MAX_TERMS];
    int n = 0;
};
int launch_repack_delta(hipStream_t st, const void* base, int base_dtype, int O, int I, int KH, int KW, int Ipad, int geglu_interleave,
                        float scale_p, const DeltaArgs& da, bf16_t* out);
// the same sum on a plain matrix (k_merge_delta): out [O][I] row-major of out_dtype (0 fp32, 1 bf16, 2 fp16 - in BOTH storage
// flavours) = round_out(base + sum_j s[j] D_j), no interleave, no pad columns, no folded factor.  I % 4 == 0; out must not overlap
// base or an operand.  What a host module outside the native store (the CLIP text encoder) gets its per-request adapters with.
int launch_merge_delta(hipStream_t st, const void* base, int base_dtype, int O, int I, const DeltaArgs& da, void* out, int out_dtype);
// out[a][c][t] = sum_b core[a][b][t] * right[b][c]  (fp32, b ascending): a Tucker core folded into the right operand of a term
int launch_lyco_core(hipStream_t st, const void* core, int core_dtype, const void* right, int right_dtype, int A, int B, int C, int T,
                     float* out);

// ---- T2I-adapter element-wise ops (kernels_t2i.hip) ----------------------------
// x NCHW [B][c][H][W] of a runtime dtype (H, W multiples of 8) -> y NHWC storage [B][H/8][W/8][64 c], channel c*64 + dy*8 + dx
int launch_pixel_unshuffle8(hipStream_t st, const void* x, int dtype, int B, int c, int H, int W, bf16_t* y);
// NHWC [B][H][W][C] -> [B][H/2][W/2][C] (C % 8 == 0; an odd last row / column is dropped): fp32 sum of the window, one rounding
int launch_avgpool2(hipStream_t st, const bf16_t* x, int B, int H, int W, int C, bf16_t* y);
int launch_relu(hipStream_t st, bf16_t* x, size_t n);                      // in place, n % 8 == 0
// y NCHW [B][C][HW] of a runtime dtype = the first C channels of x NHWC [B][HW][Cpad]
int launch_nhwc_to_nchw(hipStream_t st, const bf16_t* x, int B, int C, int HW, int Cpad, void* y, int dtype);

// ---- RRDBNet (ESRGAN) upscaler kernels (kernels_rdb.hip) ------------------------
// The epilogue every convolution of the net shares, fp32, in this order, one rounding to storage:
//   v = alpha * (acc + bias[n]);  if act: v = v > 0 ? v : 0.2 v;  v += beta1 * r1[pix][n];  v += beta2 * r2[pix][n]
// bias [N_live] or null; r1 / r2: NHWC slices (first element of the slice, own pixel stride) or null.  r1 may alias the output slice
// element for element.
struct RdbEpilogueArgs {
    const float* bias = nullptr; float alpha = 1.f; int act = 0;
    const bf16_t* r1 = nullptr; int ldr1 = 0; float beta1 = 0.f;
    const bf16_t* r2 = nullptr; int ldr2 = 0; float beta2 = 0.f;
};
void rdb_tile(int* th, int* tw);                        // output tile of k_rdb_conv (pixels)
size_t rdb_wpack_bytes(int NT, int Cin);                // bytes of the chunk-ordered weight copy
// wd [Cin / 32][9][NT][32] <- W [rows][9][Cin] (the library's conv layout), zero rows above `rows` (<= NT)
int launch_rdb_wpack(hipStream_t st, const bf16_t* W, int rows, int Cin, int NT, bf16_t* wd);
// 3x3 / stride 1 / zero padding 1 convolution over the first Cin channels (Cin % 32 == 0) of x NHWC [B][H][W] with pixel stride ldx,
// ups: nearest 2x of x inside the gather (output 2H x 2W); NT = 32 or 64 weight rows in wd, of which the first N_live are written to
// out[pix][0 .. N_live) (out: first element of the slice, pixel stride ldo) - every other byte of the buffer keeps its bits.
// GYRE_ERR_UNSUPPORTED outside the domain (NT, Cin % 32, strides % 8, 16-byte alignment, grid limits), nothing written.
int launch_rdb_conv(hipStream_t st, const bf16_t* x, int ldx, int Cin, int B, int H, int W, int ups, const bf16_t* wd, int NT,
                    int N_live, bf16_t* out, int ldo, const RdbEpilogueArgs& e);
// launch_rdb_conv's argument checks alone (no device call): 0, or the status and message the launch would refuse with
int rdb_conv_check(const bf16_t* x, int ldx, int Cin, int B, int H, int W, int ups, const bf16_t* wd, int NT, int N_live,
                   const bf16_t* out, int ldo, const RdbEpilogueArgs& e);
// the same epilogue in place over a stored slice x[pix][0 .. N_live), npix pixels of stride ldo (acc = the stored value)
int launch_rdb_epilogue(hipStream_t st, bf16_t* x, int ldo, int N_live, size_t npix, const RdbEpilogueArgs& e);
// x NCHW [B][c][H][W] of a runtime dtype -> y NHWC storage [B][H / r][W / r][rdb_unshuffle_channels(c, r)] in
// torch.nn.functional.pixel_unshuffle(r) channel order, r = 1, 2 or 4, zero channels up to the next multiple of 32
int launch_rdb_copy(hipStream_t st, const bf16_t* src, int lds, bf16_t* dst, int ldd, int C, size_t npix);   // dst[pix][0:C) = src[pix][0:C)
int rdb_unshuffle_channels(int c, int r);
int launch_pixel_unshuffle(hipStream_t st, const void* x, int dtype, int B, int c, int H, int W, int r, bf16_t* y);

// ---- SwinIR upscaler kernels (kernels_swin.hip) ---------------------------------
// Shifted-window attention over 8 x 8 windows, head dim 30 stored as 32 (arithmetic and layouts: header of kernels_swin.hip).
//   qkv [B H W][ld_qkv] token order, q / k / v of head h at columns 32 h / 32 (heads + h) / 32 (2 heads + h); o [B H W][ld_o], head h
//   written at [30 h, 30 h + 30) and nothing else; bias: launch_win_bias's output; shift 0 or 4 (0 when H == 8 or W == 8).
// The scale 30^-1/2 is applied to the fp32 dot products inside the kernel: the stored q weights and bias are the checkpoint's own.
// GYRE_ERR_UNSUPPORTED / GYRE_ERR_INVALID outside the domain, nothing written.
int win_attn_check(const bf16_t* qkv, int ld_qkv, const bf16_t* o, int ld_o, const float* bias, int B, int H, int W, int heads, int shift);
int launch_win_attn(hipStream_t st, const bf16_t* qkv, int ld_qkv, bf16_t* o, int ld_o, const float* bias, int B, int H, int W, int heads,
                    int shift);
// relative_position_bias_table [225][heads] fp32 -> the expanded bias [heads][64 x 64] fp32 in the kernel's register order
int launch_win_bias(hipStream_t st, const float* table, int heads, float* out);
// LayerNorm over the first C channels of rows with stride ldx (C <= 512); y rows of stride ldy <= 512: normalised in [0, C), zero in [C, ldy)
int launch_ln_live(hipStream_t st, const bf16_t* x, int ldx, size_t M, int C, const float* gamma, const float* beta, float eps, bf16_t* y,
                   int ldy);
// in place over n contiguous elements (n % 8 == 0): mode 0 erf GELU, mode 1 leaky ReLU of the given slope (the net uses 0.2 and 0.01)
int launch_swin_act(hipStream_t st, bf16_t* x, size_t n, int mode, float slope);
// entry: x NCHW [B][3][HW] runtime dtype -> y NHWC storage [B][HW][8] = (x - mean[c]) * range, channels 3 .. 7 zero
// exit:  x NHWC storage [B][HW][ldx]     -> y NCHW [B][3][HW] runtime dtype = x / range + mean[c]
int launch_swin_entry(hipStream_t st, const void* x, int dtype, int B, size_t HW, const float* mean3, float range, bf16_t* y);
int launch_swin_exit(hipStream_t st, const bf16_t* x, int ldx, int B, size_t HW, const float* mean3, float range, void* y, int dtype);

// ---- HAT upscaler kernels (kernels_hat.hip) --------------------------------------
// Window attention over 16 x 16 windows, head dim 30 stored as 32, the qkv / o layouts of launch_win_attn (arithmetic: header of
// kernels_hat.hip).  table: the relative-position table itself, fp32 [961][heads] (SA) or [1521][heads] (OCA); nothing is expanded.
//   HAT_ATTN_SA   256 queries x 256 keys of one window under shift 0 or 8 (always honoured, also on one window per side)
//   HAT_ATTN_OCA  256 queries x the 24 x 24 keys around the window, zero k / v outside the image; shift must be 0
// GYRE_ERR_UNSUPPORTED / GYRE_ERR_INVALID outside the domain, nothing written.
enum { HAT_ATTN_SA = 0, HAT_ATTN_OCA = 1 };
int hat_attn_check(const bf16_t* qkv, int ld_qkv, const bf16_t* o, int ld_o, const float* table, int mode, int B, int H, int W, int heads,
                   int shift);
int launch_hat_attn(hipStream_t st, const bf16_t* qkv, int ld_qkv, bf16_t* o, int ld_o, const float* table, int mode, int B, int H, int W,
                    int heads, int shift);
// pool[b][c] = mean over HW of x[b][.][c], c < C <= 256, fp32, in a fixed two-stage order (64-row chunks, then the chunks in order):
// a sample's result does not depend on B.  partial: chan_pool_partial_floats(B, HW, C) floats of scratch
size_t chan_pool_partial_floats(int B, size_t HW, int C);
int launch_chan_pool(hipStream_t st, const bf16_t* x, int ld, int B, size_t HW, int C, float* partial, float* pool);
// s[b][c] = scale * sigmoid(w2[c] . relu(w1 pool[b] + b1) + b2[c]) for c < C, 0 for C <= c < ld_s; w1 [Cs][C], w2 [C][Cs] fp32, Cs <= 8
int launch_chan_gate(hipStream_t st, const float* pool, int B, int C, int Cs, const float* w1, const float* b1, const float* w2,
                     const float* b2, float scale, float* s, int ld_s);
// y[b][p][c] += c2[b][p][c] * s[b][c] over c < Cn (a multiple of 8, <= ld_s), one fma and one rounding per element
int launch_scale_add(hipStream_t st, bf16_t* y, int ldy, const bf16_t* c2, int ldc, const float* s, int ld_s, int B, size_t HW, int Cn);
// PixelShuffle(2) on NHWC: out[b][2 y + i][2 x + j][c] = x[b][y][x][4 c + 2 i + j], c < Co (a multiple of 8); bit copies
int launch_pixel_shuffle2(hipStream_t st, const bf16_t* x, int ld_x, int B, int H, int W, int Co, bf16_t* out, int ld_out);

// ---- token-sequence T2I kernels (kernels_seq.hip) ---------------------------------
// Multi-head self-attention over the packed in_proj output (arithmetic and layouts: header of kernels_seq.hip).
//   qkv [N L][ld_qkv] sample-major rows, q / k / v of head h at columns h D / heads D + h D / 2 heads D + h D; o [N L][ld_o], head h
//   written at [h D, h D + D) of the N L rows and nothing else.  No mask, no bias; the scale D^-1/2 multiplies the fp32 dot products.
// D = 32, 64, 96 or 128 and L <= seq_attn_max_len(D) (K and V of one head in LDS: 1120 / 576 / 384 / 288); GYRE_ERR_UNSUPPORTED beyond,
// GYRE_ERR_INVALID for bad arguments, nothing written either way.  seq_attn_max_len is 0 for a head dim that is not built.
int seq_attn_max_len(int D);
int seq_attn_check(const bf16_t* qkv, int ld_qkv, const bf16_t* o, int ld_o, int N, int L, int heads, int D);
int launch_seq_attn(hipStream_t st, const bf16_t* qkv, int ld_qkv, bf16_t* o, int ld_o, int N, int L, int heads, int D);
// x sigmoid(1.702 x) in place over n contiguous elements (n % 8 == 0), fp32, one rounding
int launch_quick_gelu(hipStream_t st, bf16_t* x, size_t n);
// out[n][c] = silu(mean over HW of x[n][c][.]) of an NCHW storage map, rounded once (rows of stride ld_out >= C); fixed summation order
int launch_fuser_pool(hipStream_t st, const bf16_t* x, int N, int C, size_t HW, bf16_t* out, int ld_out);
// out[n][c][.] = x[n][c][.] (alpha[n][c] + 1), or += with accumulate = 1, over NCHW storage maps; alpha fp32 rows of stride ld_a >= C
int launch_fuser_gain(hipStream_t st, const bf16_t* x, const float* alpha, int ld_a, int N, int C, size_t HW, bf16_t* out, int accumulate);
// The token passes of the two graphs (model_t2i_seq.hip), element strides throughout, boundary dtypes 0 f32 / 1 bf16 / 2 f16:
// dst[n][r][c] = ((src[n][r][c] + add0[c]) + add1[r][c]) for n < N, r < R, c < W; src, add0 [W] and add1 [R][W] each optional; fp32
// sums in that order, one rounding.  Copies and converts rows (concat, gather), writes broadcast embedding rows, adds embeddings.
struct SeqRows {
    const void* src = nullptr; int src_dtype = 0; size_t src_ss = 0, src_rs = 0;      // sample stride, row stride
    const float* add0 = nullptr; const float* add1 = nullptr;
    void* dst = nullptr; int dst_dtype = 0; size_t dst_ss = 0, dst_rs = 0;
    int N = 0, R = 0, W = 0;
};
int launch_seq_rows(hipStream_t st, const SeqRows& a);
// out[n][t][c] = tok[n][t][c] (g[n][t][c] + 1): tok [N][T][W] contiguous and out (sample stride out_ss, row stride W) of `dtype`, g storage
// (sample stride g_ss, row stride W); the sum and the product round in fp32 on their own, then one rounding to out
struct SeqTokenGain {
    const void* tok = nullptr; const bf16_t* g = nullptr; size_t g_ss = 0; void* out = nullptr; size_t out_ss = 0; int dtype = 0;
    int N = 0, T = 0, W = 0;
};
int launch_seq_token_gain(hipStream_t st, const SeqTokenGain& a);
// dst[c][r] = src[r][c]: a parameter used as x @ P, P [R][Cc] of a runtime dtype, into the row-major [Cc][i_pad] the GEMMs read
int launch_repack_transposed(hipStream_t st, const void* src, int dtype, int R, int Cc, int i_pad, bf16_t* dst);

// ---- line-art hinter kernels (kernels_inorm.hip) ----------------------------------
// Instance normalisation over NHWC rows [B][HW] of stride ld (C = 64, 128 or 256 live channels): stats [B][C][2] = (mean, rstd) with the
// biased variance, fp32, shifted sums in a fixed order (512-row chunks, then the chunks in eight interleaved slices, then the slices): a sample's statistics do
// not depend on B.  partial: inorm_partial_floats(B, HW, C) floats of scratch
size_t inorm_partial_floats(int B, size_t HW, int C);
int launch_inorm_stats(hipStream_t st, const bf16_t* x, int ld, int B, size_t HW, int C, float eps, float* partial, float* stats);
// out = relu?((x - mean) * rstd) (+ res), fp32, one rounding, over the logical image [B][H][W][C] (dense, pixel stride C):
//   shuffled  x is [B][H/2][W/2][(a, b, C)], pixel (2i + a, 2j + b) at row (i, j), columns (2a + b) C + c (a sub-pixel transposed conv's output)
//   res       an image of the same logical size stored with a border of res_pad pixels, [B][H + 2 res_pad][W + 2 res_pad][C]
//   pad       0, 1 or 3 (< H, W): out is [B][H + 2 pad][W + 2 pad][C] with nn.ReflectionPad2d's mirrored border
//   patch     out is [B][H][W][4 C]: row (y, x) holds pixels (y + dy, x + dx) in (dy, dx, c) order, zeros past the last row / column (pad 0)
struct InormApply {
    const bf16_t* x = nullptr; const float* stats = nullptr; const bf16_t* res = nullptr; bf16_t* out = nullptr;
    int B = 0, H = 0, W = 0, C = 0;
    int shuffled = 0, relu = 0, res_pad = 0, pad = 0, patch = 0;
};
int inorm_apply_check(const InormApply& a);              // the launch's argument checks alone (no device call)
int launch_inorm_apply(hipStream_t st, const InormApply& a);
// ConvTranspose2d(k 3, s 2, p 1, output_padding 1) weight [Cin][Cout][3][3] of a runtime dtype -> out [4 Cout][4 Cin] storage: rows
// (a, b, co) of the output parity, columns (dy, dx, ci) of the 2x2 source patch; a = 0: ky = 1 at dy = 0; a = 1: ky = 2 at dy = 0, ky = 0
// at dy = 1 (columns alike); the other 7 of the 16 blocks are zero
int launch_tconv_compose(hipStream_t st, const void* w, int dtype, int Cin, int Cout, bf16_t* out);
// 7x7 / reflection padding 3 convolution of x NHWC [B][H][W][8] (3 live channels) into 64 channels: Wt [64][7][7][8], bias [64], out
// NHWC [B][H][W][64]; H, W >= 4
int launch_conv7_in(hipStream_t st, const bf16_t* x, int B, int H, int W, const bf16_t* Wt, const float* bias, bf16_t* out);
// 7x7 / no padding convolution of xp NHWC [B][Ho + 6][Wo + 6][64] into ONE channel: Wt [7][7][64], bias [1], optional sigmoid, out NCHW
// [B][1][Ho][Wo] of a runtime dtype
int launch_conv7_out(hipStream_t st, const bf16_t* xp, int B, int Ho, int Wo, const bf16_t* Wt, const float* bias, int sigmoid,
                     void* out, int out_dtype);

// ---- HED edge-detector kernels (kernels_hed.hip) ------------------------------------
// entry: x NCHW [B][3][H][W] of a runtime dtype -> y NHWC storage [B][H + 68][W + 68][8]: the image inside a zero border of HED_BORDER
// pixels, channels 3 .. 7 zero (conv1_1's padding 35 = this border + the planner's padding 1)
constexpr int HED_BORDER = 34;
int launch_hed_entry(hipStream_t st, const void* x, int dtype, int B, int H, int W, bf16_t* y);
// The end of a VGG stage over its last convolution BEFORE the ReLU, x NHWC [B][Hs][Ws][C], C = 64 / 128 / 256 / 512, read once:
//   pool [B][ceil(Hs / 2)][ceil(Ws / 2)][C] = relu(max over the 2x2 ceil-mode window), exact; null: not written (stage 5)
//   so   [B][Hs][Ws] fp32 = bias[0] + sum_c w[c] relu(x[c]), fp32 in an order that depends on C alone
int hed_tail_check(const bf16_t* x, int B, int Hs, int Ws, int C, const float* w, const float* bias, const bf16_t* pool, const float* so);
int launch_hed_tail(hipStream_t st, const bf16_t* x, int B, int Hs, int Ws, int C, const float* w, const float* bias, bf16_t* pool, float* so);
// out [6][B][1][H][W] of out_dtype = sigmoid of (so1 .. so5 cropped, their fuse): so[0] [B][Hk[0]][Wk[0]] read at (y + oy[0], x + ox[0]);
// so[k], k = 1 .. 4, through the bilinear transposed convolution of kernel 2 s and stride s = 1 << k, whose (Hk[k] + 1) s image is read
// at (y + oy[k], x + ox[k]); fuse = bf[0] + sum_k wf[k] l_k.  All fp32, one rounding.
struct HedFuse {
    const float* so[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int Hk[5] = {0, 0, 0, 0, 0}, Wk[5] = {0, 0, 0, 0, 0}, oy[5] = {0, 0, 0, 0, 0}, ox[5] = {0, 0, 0, 0, 0};
    const float* wf = nullptr; const float* bf = nullptr;
    void* out = nullptr; int out_dtype = 0;
    int B = 0, H = 0, W = 0;
};
int hed_fuse_check(const HedFuse& a);                    // the launch's argument checks alone (no device call)
int launch_hed_fuse(hipStream_t st, const HedFuse& a);

// ---- MLSD line-detector kernels (kernels_mlsd.hip) ----------------------------------
// BatchNorm (eval, eps 1e-5) folded into a convolution in fp32: out = storage(w gamma / sqrt(var + eps)), bias = beta + (conv_bias - mean)
// gamma / sqrt(var + eps).  w: the PyTorch weight [O][I][k][k] as fp32 (depthwise: [O][1][3][3]); conv_bias may be null.  Destination:
//   DENSE      [o_pad][taps][i_pad], taps 1 or 9 (the planner's order), zero in the padding
//   DEPTHWISE  [9][o_pad]
//   ENTRY      [9][I][o_pad]
// bias [o_pad] fp32, zero in the padding
enum { MLSD_FOLD_DENSE = 0, MLSD_FOLD_DEPTHWISE = 1, MLSD_FOLD_ENTRY = 2 };
struct MlsdFold {
    const float *w = nullptr, *conv_bias = nullptr, *gamma = nullptr, *beta = nullptr, *mean = nullptr, *var = nullptr;
    bf16_t* out = nullptr; float* bias = nullptr;
    int kind = 0, O = 0, I = 0, taps = 1, o_pad = 0, i_pad = 0;
};
int launch_mlsd_fold(hipStream_t st, const MlsdFold& a);
// y [B][H / 2][W / 2][32] = relu6(conv3x3 stride 2 (x NCHW [B][4][H][W] of dtype) + bias), zero padding on the right / bottom only;
// w [9][4][32] storage
int launch_mlsd_entry(hipStream_t st, const void* x, int dtype, int B, int H, int W, const bf16_t* w, const float* bias, bf16_t* y);
// y = relu6(depthwise3x3(x) + bias) over NHWC [B][H][W][C], C % 8 == 0, w [9][C] storage, bias [C]: stride 1 / zero padding 1 ->
// [B][H][W][C], stride 2 / right-bottom padding -> [B][H / 2][W / 2][C].  relu6_in: relu6 is applied to x as it is read
int launch_mlsd_dw(hipStream_t st, const bf16_t* x, int B, int H, int W, int C, const bf16_t* w, const float* bias, int stride, int relu6_in,
                   bf16_t* y);
// y[b][oy][ox][0 .. C) (pixel stride ldy) = bilinear x2, align_corners=True, of x [B][H][W] (pixel stride ldx); relu_in: relu on the reads
int launch_mlsd_up2(hipStream_t st, const bf16_t* x, int B, int H, int W, int C, int ldx, int relu_in, bf16_t* y, int ldy);
// y = relu(conv3x3 dilation 5 / zero padding 5 (x) + bias), NHWC [B][H][W][64] -> the same, w [64][9][64] storage
int launch_mlsd_dconv(hipStream_t st, const bf16_t* x, int B, int H, int W, const bf16_t* w, const float* bias, bf16_t* y);
// in place: relu (relu6) over the first C channels of `rows` rows of pitch ld; y = relu(y) + x over n contiguous elements
int launch_mlsd_act(hipStream_t st, bf16_t* x, size_t rows, int C, int ld, int relu6);
int launch_mlsd_relu_add(hipStream_t st, bf16_t* y, const bf16_t* x, size_t n);
// out NCHW [B][9][H][W] of out_dtype = channels 7 .. 15 of x NHWC [B][H][W][16]
int launch_mlsd_exit(hipStream_t st, const bf16_t* x, int B, int H, int W, void* out, int out_dtype);

// ---- ControlNet element-wise ops (kernels_ctrl.hip) ----------------------------
int launch_silu(hipStream_t st, bf16_t* x, size_t n);                      // x * sigmoid(x) in place, n % 8 == 0
// out NCHW [out_B][C][HW] of a runtime dtype <- scale * f, f NHWC storage [B][HW][Cpad] (first C channels), samples [out_b0, out_b0 + B):
// accumulate == 0 assigns and writes every other sample of `out` as zero, accumulate == 1 adds and leaves the others alone
int launch_ctrl_emit(hipStream_t st, const bf16_t* f, int B, int C, int HW, int Cpad, float scale, int accumulate, void* out,
                     int out_dtype, int out_B, int out_b0);
// the same with every product times mask[mask_B == 1 ? 0 : b][p] (fp32 [mask_B][HW]): out = rnd(fl(fl(scale f) m) [+ old]); mask ==
// nullptr is launch_ctrl_emit
int launch_ctrl_emit_masked(hipStream_t st, const bf16_t* f, int B, int C, int HW, int Cpad, float scale, int accumulate, void* out,
                            int out_dtype, int out_B, int out_b0, const float* mask, int mask_B);

// ---- MFMA GEMM / implicit-GEMM conv (kernels_gemm.hip) -------------------------
enum { GEMM_LINEAR = 0, GEMM_CONV3 = 1 };
enum { OUT_BF16 = 0, OUT_NCHW = 1, OUT_BF16_T = 2 };
struct GemmParams {
    // A operand: [M][K] rows (linear) or NHWC image gathered through a 3x3 window (conv)
    const bf16_t* A = nullptr; const bf16_t* A2 = nullptr; int C1 = 0;  // dual source split along K / channel
    int lda = 0, lda2 = 0;      // row (pixel) stride of each source, elements
    int mode = GEMM_LINEAR;
    int Hi = 0, Wi = 0, Cin = 0;  // conv: SOURCE spatial dims (before the fused 2x upsample) and channels (multiple of 8)
    int Ho = 0, Wo = 0, stride = 1, pad = 1, ups = 0;
    // B operand: W[N][K] bf16, K contiguous
    const bf16_t* W = nullptr; int K = 0; int N = 0; int M = 0;
    // epilogue
    const float* bias = nullptr;      // [N] (GEGLU: [2N] interleaved like the weight rows)
    const float* rowbias = nullptr;   // [M / rows_per_sample][ld_rowbias], per-sample per-channel (time embedding)
    int rows_per_sample = 1; int ld_rowbias = 0;
    const bf16_t* residual = nullptr; int ldr = 0;
    int geglu = 0;                    // W has 2*N_out rows interleaved in 16-row value/gate groups; N == 2*N_out
    void* out = nullptr; int ldc = 0; int out_mode = OUT_BF16; int out_dtype = 1;
    int tokens_per_batch = 0; int ldt = 0;  // OUT_BF16_T: out[(b*N + col)*ldt + tok]
    // fused Q|K|V projection (8-wave kernels, OUT_BF16): columns >= vt_col0 are written transposed to
    // vt_out[(b*(N - vt_col0) + col - vt_col0)*ldt + tok] instead of `out` (V^T for the attention kernel)
    bf16_t* vt_out = nullptr; int vt_col0 = 0;
    const bf16_t* zero_page = nullptr;      // >= 16 zero bytes in global memory (filled in by launch_gemm)
    int force_cfg = 0;                      // tests/tuning: 0 auto, else tile-config id (see launch_gemm)
    int debug = 0;                          // tuning ablations: bit0 = no operand loads in the K loop, bit1 = no MFMAs
    int Hup = 0, Wup = 0;         // ups: logical size of the upsampled image (0 = 2*Hi x 2*Wi); < 2x crops the last row/col
    int samples = 0;              // batch entries folded into M (0 = unknown); used by the batch-invariant planner
    float* splitk_ws = nullptr; size_t splitk_ws_bytes = 0;  // fp32 partial slabs [splits][M][N] (see gemm_plan)
    // batched form (4-wave kernels only): problem b uses A + b*bsA, W + b*bsW, out + b*bsC (element strides); no bias /
    // residual / split-K.  Used for the per-sample token-similarity matrix of ToMe.
    int batch = 1; size_t bsA = 0, bsW = 0, bsC = 0;
    // LayerNorm folded into the GEMM (8-wave kernels, linear mode, one source, no split-K): A holds the RAW rows, W the
    // gamma-scaled weights W'[n][k] = W[n][k] * gamma[k], bias[n] = sum_k beta[k] W[n][k] (+ the layer's bias),
    // ln_colsum[n] = sum_k W'[n][k] (launch_ln_fold) and ln_stats[m] = (rstd, rstd * mean) of row m
    // (launch_layernorm_stats, one streaming read of the rows).  The epilogue applies
    // out = rstd * acc - rstd * mean * colsum + bias: the normalised tensor is never written or re-read.
    // (Accumulating the row sums inside the K loop from the operand fragments - v_dot2c_f32_bf16, no extra pass - was built
    // and measured: every N tile repeats the sums at ~20 cycles per packed pair, slower than the separate statistics pass
    // for every layer of the UNet; profiles/README.md.)
    const float* ln_colsum = nullptr; const float* ln_stats = nullptr;
    // Statistics straight from the kernel that PRODUCED the rows: rowstat_out (8-wave kernels, staged epilogue, no GEGLU /
    // split-K / fused V^T; GemmPlan::rowstat_parts > 0) receives [tiles_n][M][2] = per row the sum and the sum of squares of the
    // bf16-rounded outputs of each N tile, reduced in a fixed order (lanes -> waves -> tile).  A consumer with the folded
    // LayerNorm takes them as ln_parts / ln_nparts instead of ln_stats and finishes mean / rstd in its epilogue
    // (variance as E[x^2] - mean^2 in fp32): the separate statistics pass disappears.
    float* rowstat_out = nullptr;
    const float* ln_parts = nullptr; int ln_nparts = 0; float ln_eps = 1e-5f;
    // GroupNorm statistics straight from the kernel that PRODUCED the tensor (the column counterpart of rowstat_out):
    // colstat_out [M / colstat_rows][N / colstat_unit][2] = per block of colstat_rows consecutive output rows and per unit of
    // colstat_unit consecutive channels the sum and the sum of squares of the bf16-rounded outputs, reduced in a fixed order
    // (rows of a 16- / 32-row slab -> slabs -> wave tiles -> channels of the unit; no atomics).  colstat_rows is dictated by
    // the kernel the planner picks: GemmPlan::colstat_rows (0: this problem cannot; the consumer then runs its own statistics
    // pass).  The row blocks never straddle a sample (rows_per_sample % colstat_rows == 0 is part of the condition), so a
    // GroupNorm over the tensor - alone or as one source of a skip concat - finishes mean / rstd from these partials
    // (GnParams::cs_x / cs_x2) and the statistics pass over the tensor disappears.
    float* colstat_out = nullptr; int colstat_unit = 0;
    // A-resident kernel (kernels_gemm_ar.hip, tile config 30: K = 320 / 640 linear problems).  It reads W from a fragment-ordered
    // copy: ar_ok = the caller can provide one (the planner only then picks the config; the model runtime packs per handle on
    // first use and sets w_packed, tests pass a scratch buffer through gyre_debug_set_ar_workspace); no_ar = the caller wants a
    // feature that kernel lacks from this launch (column statistics for a GroupNorm)
    const void* w_packed = nullptr; int ar_ok = 0, no_ar = 0;
    // BLOCKED copy of W for the LDS-DMA tile kernels (tile configs 4 - 8, 12, 20 - 24, 32; round 5): 1-KiB blocks of 8 weight rows x
    // 64 k, block (n >> 3, k >> 6) at ((n >> 3) * (K / 64) + (k >> 6)) * 512 elements, row-major inside.  A wave's LDS-DMA request
    // (8 rows x 128 B) then reads ONE contiguous KiB instead of eight lines 2 K bytes apart: tools/ubench/l2_bw.hip measures 82 - 125
    // GB/s per CU from L2 for requests that stay inside 16 KB and 19 - 60 for requests spread over more 4-KiB pages, which is what
    // every weight request with K >= 1280 (and every 3x3 conv's: K = 9 Cin) was.  K % 64 == 0, N % 8 == 0; kernels that do not
    // know the layout ignore the field and read W.  (launch_w_block makes the copy; the model runtime caches one per weight.)
    const bf16_t* W_blk = nullptr;
    // per-SAMPLE weights (8-wave tile configs 4 - 8, linear mode): rows of sample b = row / rows_per_sample read W + b *
    // w_sample_stride (elements); row blocks never straddle a sample (GemmPlan::per_sample_w).  The GroupNorm folded into a
    // Transformer2D's proj_in (launch_gn_fold); the per-sample bias travels as `rowbias`
    size_t w_sample_stride = 0;
    // 1x1 SHORTCUT folded into a 3x3 convolution as extra K steps (round 6; pipelined 256x320 tile only, stride 1, pad 1, no upsample):
    //   out = conv3x3(A | A2) + (S | S2) Wsc^T + bias        (the resnet's conv2 + conv_shortcut of a channel-changing / concat block)
    // Behind the nine taps of every 64-channel chunk of the conv input the K loop walks sc_K more channels of a second image pair
    // (same H x W as the output, split at sc_C1 like A | A2) through the CENTRE tap.  W holds [N][9 Cin + sc_K] rows (the conv's rows
    // followed by the shortcut's: launch_concat_rows), K = 9 Cin + sc_K, bias = the sum of the two biases.  GemmPlan::shortcut_fold
    // says whether launch_gemm would run `p` on a kernel that knows the form.
    const bf16_t* sc_A = nullptr; const bf16_t* sc_A2 = nullptr; int sc_lda = 0, sc_lda2 = 0, sc_C1 = 0, sc_K = 0;
    // conv: circular instead of zero padding along x (bit 0) / y (bit 1) - the reference's request option "tiling"
    // (unified_pipeline.py:1671-1712 patches every Conv2d's own padding to F.pad(mode="circular")); 4-wave tile configs only
    int wrap = 0;
    // nearest-2x upsample + 3x3 / stride 1 / pad 1 convolution as FOUR 2x2 convolutions on the SOURCE image, one per output parity
    // (a, b) = (Y & 1, X & 1): after the upsample the nine taps of an output pixel read only 2x2 distinct source pixels, window origin
    // (i - 1 + a, j - 1 + b) for the output pixel (2i + a, 2j + b), and the upsampled image's zero border is the source's.  K = 4 Cin
    // (taps t' = 2 ty + tx, chunk outer / tap inner like the nine-tap walk), M = B Ho Wo with Ho = 2 Hi, Wo = 2 Wi as before; the
    // kernel's tile rows are (parity, 256 rows of that parity's B Hi Wi source pixels) and every store goes to the output row of its
    // pixel, so out, residual, rowbias and the split-K slabs keep their natural row order.  W_blk holds the composed weights
    // (launch_compose_ups4): [4 N][4 Cin] in blocked order, rows parity * N + n; the kernel reads W_blk alone (callers set W to the same buffer: the
    // planner and the launch checks look at it for NULL and alignment only).  Pipelined 256x320 tile only
    // (GemmPlan::cfg == 24), one source, Cin % 64 == 0; column statistics: Hi Wi % 256 == 0, row block (sample, parity, local tile).
    // Set by Exec::conv3 and gyre_op_upsample_conv_test alone.
    int ups4 = 0;
};
// the composed weights of GemmParams::ups4 from W [N][9 Cin] (tap-major K): per parity (a, b) and 2x2 tap (ty, tx) the fp32 sum of the
// nine-tap weights whose upsampled pixel lands on that source pixel - rows ky in {0} | {1, 2} for a = 0, {0, 1} | {2} for a = 1,
// columns alike - ky ascending outer, kx ascending inner, one rounding to the storage type.  out: 16 N Cin elements, blocked order.
int launch_compose_ups4(hipStream_t st, const bf16_t* W, int N, int Cin, bf16_t* out);
bool gemm4s_supports(const GemmParams& p, int cfg);     // (kernels_gemm4s.hip) the pipelined tile configs' domain
// out[n][0:K1] = a[n][0:K1], out[n][K1:K1+K2] = b[n][0:K2] (bf16 rows; K1, K2 multiples of 8): the folded conv + shortcut weight
int launch_concat_rows(hipStream_t st, const bf16_t* a, int K1, const bf16_t* b, int K2, int N, bf16_t* out);
// W'[n][k] = bf16(W[n][k] * gamma[k]); colsum[n] = sum_k W'[n][k]; bias_out[n] = sum_k beta[k] * W[n][k] + (bias ? bias[n] : 0)
int launch_ln_fold(hipStream_t st, const bf16_t* W, int N, int K, const float* gamma, const float* beta, const float* bias,
                   bf16_t* Wf, float* colsum, float* bias_out);
// A-resident kernel (tile config 30): bytes of / conversion into the fragment-ordered weight copy it reads (GemmParams::w_packed)
size_t gemm_ar_packed_bytes(int N, int K);
int launch_ar_pack(hipStream_t st, const bf16_t* W, int N, int K, void* out);
int launch_w_block(hipStream_t st, const bf16_t* W, int N, int K, bf16_t* out);   // out: N * K elements (GemmParams::W_blk)
// 3x3 / stride 1 / zero padding 1 convolution of NHWC bf16 x [B][H][W][C] into O <= 16 channels, written as NCHW of the given
// runtime dtype (kernels_conv_out.hip): W [O][3][3][C] bf16, bias [O] or null.  conv_out_supports: C % 64 == 0 and the weights fit LDS.
bool conv_out_supports(int C, int O);
int launch_conv_out(hipStream_t st, const bf16_t* x, int B, int H, int W, int C, const bf16_t* Wt, const float* bias, int O,
                    void* out, int out_dtype);
// What launch_gemm will do with `p`: a pure function of the problem (and of this thread's planner state, gemm_planner_state()).
// The caller provides `ws_bytes` of split-K slabs (or none: the launch then falls back to the best single-split config).  The
// remaining fields answer the caller's questions about fusions; with a forced tile config or batch-invariant planning every
// fusion answer is "no".
struct GemmPlan {
    int cfg = 3, splits = 1;          // tile config (GemmParams::force_cfg ids) and K slices
    size_t ws_bytes = 0;
    int colstat_rows = 0;             // rows per colstat_out row block for p.colstat_unit (0: the consumer runs its own statistics pass)
    int rowstat_parts = 0;            // partial sums per row the launch leaves in rowstat_out (0: this problem cannot)
    bool ln_fold = false;             // the kernel folds a LayerNorm (ln_colsum)
    bool per_sample_w = false;        // the kernel reads per-sample weights (w_sample_stride; row blocks never straddle a sample)
    bool shortcut_fold = false;       // the kernel folds the 1x1 shortcut into the 3x3 convolution (sc_*)
    bool w_block = false;             // the kernel reads a blocked weight copy (W_blk) and the shape gains from one
    bool ar_pack = false;             // the A-resident kernel: it needs the packed weight copy (w_packed)
    int vt_align = 0;                 // fused Q|K|V: vt_col0 must be a multiple of this (0: the kernel has no transposing epilogue)
};
GemmPlan gemm_plan(const GemmParams& p);
int launch_gemm(hipStream_t st, const GemmParams& p);                          // plans `p`, then runs that plan
int launch_gemm(hipStream_t st, const GemmParams& p, const GemmPlan& plan);    // plan: gemm_plan(p)
// Plan queries (no device).  *nst = the LDS ring depth the launch of `plan` would use when its kernel is an 8-wave one (else 0),
// *uni = 1 when a convolution's K loop takes the uniform-tap form (chunk outer, tap inner), both from the rule the launch reads.
void gemm_plan_loop_form(const GemmParams& p, const GemmPlan& plan, int* nst, int* uni);
int gemm_tile_table(int* out, int cap);      // (id, bm, bn, kind) of every tile config, at most cap ints; returns the number of configs


// ---- flash-style attention (kernels_attn.hip) ------------------------------------
struct AttnParams {
    const bf16_t* q; int ldq;   // [B][Nq][ldq], head h at column h*D
    const bf16_t* k; int ldk;   // [B][Nk][ldk]
    const bf16_t* vt; int ldvt; // [B][H*D][ldvt] (V transposed: token index contiguous)
    bf16_t* o; int ldo;         // [B][Nq][ldo]
    int B, H, Nq, Nk, D;
    int k_prescaled = 0;        // K already carries log2(e)/sqrt(D) (folded into the to_k weights at repack time)
    int always_check = 0;       // tuning (k_attn3): keep the per-tile overflow check instead of the optimistic first pass
    unsigned* redo_counter = nullptr;   // incremented by every workgroup that repeats its pass (per device; gyre_debug_attn_redo_count)
};
// Values of gyre_debug_force_attn_variant (bits 0 .. 7; bits 8 and up: the ablation id of GYRE_ATTN_ABLATIONS builds).
enum AttnVariant {
    ATTN_VAR_AUTO = 0,           // the rule of attn_plan()
    ATTN_VAR_V1 = 1,             // k_attn
    ATTN_VAR_V2_PLAIN = 2,       // k_attn2, plain online softmax
    ATTN_VAR_V2_FOLD = 3,        // k_attn2 FOLD where K is prescaled and the head dim has the form
    ATTN_VAR_V2_Q64 = 4,         // k_attn2 plain with 64 query rows per wave (QI = 4; D <= 32)
    ATTN_VAR_V3 = 5,             // k_attn3 whatever the key count
    ATTN_VAR_NO_QLOOP = 6,       // automatic, without the several-query-blocks-per-workgroup form of short key sequences
    ATTN_VAR_ALWAYS_CHECK = 7,   // automatic, k_attn3 with the per-tile overflow check from the start
    ATTN_VAR_AUTO_ALIAS = 8,     // a synonym of 0, kept for the tools
};
enum AttnFamily { ATTN_FAM_V1 = 0, ATTN_FAM_V2_PLAIN = 1, ATTN_FAM_V2_FOLD = 2, ATTN_FAM_V3 = 3 };
// What one launch_attention call runs, decided once on the host (no HIP call, no global state).
struct AttnPlan {
    int status = 0; std::string error;       // status != 0: the launch is refused with this code and message
    int family = 0, D = 0, QI = 0, row = -1; // AttnFamily; row of the launch table (kernels_attn.hip)
    int PD = 0, slots = 0, stage_bytes = 0;  // LDS-DMA ring: lookahead, slot count, bytes per slot (0 for k_attn)
    int lds_bytes = 0;                       // dynamic LDS of the launch
    dim3 grid;
    bool qloop = false; int qiter = 1;       // k_attn2: query blocks per workgroup
    bool always_check = false;               // k_attn3: AttnParams::always_check of the launch
    int ablation = 0;                        // GYRE_ATTN_ABLATIONS builds (k_attn3, D = 40)
    double flops = 0, bytes = 0;             // the profiling scope's model
};
AttnPlan attn_plan(const AttnParams& p, int variant);
constexpr int ATTN_PLAN_INTS = 12, ATTN_BWD_PLAN_INTS = 10;     // gyre_debug_attn_plan / gyre_debug_attn_bwd_plan (include/gyre_hip.h)
int launch_attention(hipStream_t st, const AttnParams& p);

// ---- fused cross-attention block: to_q (+ folded LayerNorm) -> attention over the cached text keys -> to_out + residual (kernels_xattn.hip) ----
struct XattnParams {
    const bf16_t* x; int ldx;                 // [M][C] rows BEFORE the LayerNorm (also the residual)
    const bf16_t* wq;                         // gamma-folded to_q weights [C][C] (launch_ln_fold)
    const float* q_colsum; const float* q_bias;       // [C] colsum of W', folded bias
    const float* ln_parts; int ln_nparts; const float* ln_stats; float ln_eps;
    const bf16_t* k; const bf16_t* vt; int ldvt;     // context cache: K [B][Nk][C] (prescaled), V^T [B][C][ldvt]
    const bf16_t* wo; const float* bo;       // to_out [C][C], [C]
    bf16_t* out; int ldo;                     // [M][C]
    float* rowstat_out;                       // [M][2] (one partial per row) or null
    int M, rows_per_sample, Nk, heads;
};

bool xattn_supports(int C, int heads, int Nq, int Nk, int M);
int launch_xattn(hipStream_t st, const XattnParams& p, int C);

// ---- input-gradient kernels of the CLIP-guided mode (kernels_bwd.hip) ---------------------------------------------
struct GnBwdParams {
    const bf16_t* x; const bf16_t* x2; int C1;       // forward input (x2 = second source of the skip concat, or null)
    int B, HW, C, G;
    const float* gamma; const float* beta; float eps; int silu;
    const bf16_t* dy;                                // [B][HW][C]
    const bf16_t* addend;                            // optional [B][HW][C1], added to dx (identity-shortcut gradient)
    bf16_t* dx; bf16_t* dx2;                         // [B][HW][C1], [B][HW][C - C1]
    // filled in by launch_groupnorm_bwd from its workspace
    float* partial = nullptr; const float* fwd_partial = nullptr; int nchunks = 0;
};
size_t gn_bwd_workspace_bytes(int B, int HW, int C, int G);
int launch_groupnorm_bwd(hipStream_t st, GnBwdParams p, void* ws);
int launch_layernorm_bwd(hipStream_t st, const bf16_t* x, const bf16_t* dy, int M, int C, const float* gamma, float eps,
                         const bf16_t* addend, bf16_t* dx);
// pre: [M][2F] GEGLU pre-activation in the interleaved column order of the packed weight; dy: [M][F]; dpre: [M][2F]
int launch_geglu_bwd(hipStream_t st, const bf16_t* pre, const bf16_t* dy, size_t M, int F, bf16_t* dpre);
int launch_pool2_sum(hipStream_t st, const bf16_t* du, int B, int H, int W, int Hu, int Wu, int C, bf16_t* dx);
int launch_zero_stuff2(hipStream_t st, const bf16_t* dy, int B, int Ho, int Wo, int H, int W, int C, bf16_t* dz);
int launch_add_bf16(hipStream_t st, bf16_t* y, const bf16_t* x, size_t n);
int launch_conv_weight_t(hipStream_t st, const bf16_t* w, int O, int I, bf16_t* wt);   // [O][9][I] -> [I][9][O], window rotated
int launch_transpose(hipStream_t st, const bf16_t* in, int ld_in, int R, int C, bf16_t* out, int ld_out, int batch,
                     size_t bs_in, size_t bs_out);
struct AttnBwdParams {
    const bf16_t* q; int ldq;      // [B][Nq][ldq], head h at column h*D
    const bf16_t* k; int ldk;      // [B][Nk][ldk]
    const bf16_t* v; int ldv;      // [B][Nk][ldv]  (row-major, unlike the forward kernel's V^T)
    const bf16_t* o; int ldo;      // forward output [B][Nq][ldo]
    const bf16_t* d_o; int lddo;   // its gradient
    const bf16_t* kt; int ldkt;    // K transposed [B][H*D][ldkt], ldkt >= Nk rounded up to 32, pad columns zero
    const bf16_t* qt; const bf16_t* d_ot; int ldqt;   // Q^T, dO^T [B][H*D][ldqt] (only read when dk != null)
    bf16_t* dq; int lddq;
    bf16_t* dk; int lddk; bf16_t* dv; int lddv;       // dk == null: queries only (cross-attention: the context gets no gradient)
    void* stats;                   // attn_bwd_stats_bytes(B, H, Nq)
    int B, H, Nq, Nk, D;
    int k_prescaled;               // K carries log2(e)/sqrt(D) (see AttnParams)
    // filled in by launch_attention_bwd
    float* lse = nullptr; float* delta = nullptr; int NqPad = 0; float alpha = 0.f, beta = 0.f;
};
size_t attn_bwd_stats_bytes(int B, int H, int Nq);
bool attn_bwd_needs_transposes(int D);     // false: the LDS-tiled kernels (D <= 160) ignore kt / qt / d_ot
int launch_attention_bwd(hipStream_t st, AttnBwdParams p);
int attn_bwd_table(int which, int32_t* out, int cap);      // gyre_debug_attn_tables: 1 = LDS-tile rows, 2 = register-staged rows

// ---- ToMe: bipartite soft matching + merge of self-attention K / V tokens (kernels_tome.hip) ---------------------------
struct TomeParams {
    const bf16_t* k; int ldk;     // [B][N][ldk]  keys (row-major; any column offset already applied)
    const bf16_t* v; int ldv;     // [B][N][ldv]  values (row-major)
    int B, N, C, r;               // r tokens of the "a" half (even tokens) are merged into their best "b" (odd) match
    bf16_t* k_out;                // [B][N - r][C]
    bf16_t* vt_out; int ldvt;     // [B][C][ldvt]  merged values, transposed (what the attention kernel streams)
    void* ws; size_t ws_bytes;    // tome_workspace_bytes(B, N, C)
    int* order_out = nullptr;     // optional [B][N/2]: a-token indices by descending best-match score
    int* node_idx_out = nullptr;  // optional [B][N/2]: best b match of every a token
    bf16_t* vrows_out = nullptr;  // optional [B][N - r][C]: merged values row-major (the backward pass reads rows)
    int* dstlist_out = nullptr;   // optional [B][N/2]: entry k < r = b token the k-th ranked a token was merged into
};
size_t tome_workspace_bytes(int B, int N, int C);
int tome_effective_r(int N, int r);       // min(r, N / 2), 0 when N < 2
int launch_tome_merge(hipStream_t st, const TomeParams& p);
// adjoint of the merge for one merged tensor: dy [B][N - r][C] -> dx [B][N][ldx] (every original token receives the gradient
// of the row it went into, divided by that row's token count); order / dstlist from launch_tome_merge, inv: int scratch [B][N/2]
int launch_tome_unmerge(hipStream_t st, const bf16_t* dy, int B, int N, int C, int r, const int* order, const int* dstlist,
                        int* inv, bf16_t* dx, int ldx);
