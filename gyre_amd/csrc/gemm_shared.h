// Pieces shared by the GEMM translation units (kernels_gemm.hip: 4-/8-wave kernels, kernels_gemm4s.hip: the
// one-wave-per-SIMD kernel).
#pragma once
#include "kernels.h"

#define BK 64

typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_void_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

// XCD-aware, bijective tile order: blocks b, b+8, ... run on the same XCD (private L2); give each XCD a
// contiguous chunk of tile ids, tile id -> (tm, tn) with tn fastest so neighbours share the A rows.
__device__ __forceinline__ int xcd_tile_id(int bid, int ntiles) {
    const int q = ntiles >> 3, r = ntiles & 7;
    const int xcd = bid & 7, loc = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
}

// 256-byte zero page per device: source of the zero padding for the LDS-DMA kernels (read-only after creation)
const bf16_t* gemm_zero_page_for_current_device();

int launch_splitk_reduce(hipStream_t st, const GemmParams& p, int splits);   // kernels_gemm.hip

// The tile configs (GemmParams::force_cfg ids) and what each kernel can do (table in kernels_gemm.hip).  Every fusion goes through
// an epilogue that needs gemm_staged_epilogue_ok(p): the 8-wave kernels' LDS-staged one; the pipelined, A-resident and
// small-problem kernels take only problems that satisfy it.
enum GemmKind { GEMM_K_4W, GEMM_K_8W, GEMM_K_4S, GEMM_K_AR, GEMM_K_SM };   // register-staged 4-wave, LDS-DMA 8-wave, pipelined,
                                                                             // A-resident, small-problem
struct GemmTile {
    int id, bm, bn; GemmKind kind;
    bool geglu;          // pairs GEGLU value / gate columns (an even fragment count per wave)
    int vt_align;        // fused Q|K|V: the V columns start on a multiple of this wave-tile width (0: no transposing epilogue)
    int cs_rows;         // column statistics of the unsplit kernel: rows per row block (0: none)
    bool rowstats;       // row statistics: one partial per bn-wide N tile (A-resident kernel: per N-range split, gemm_ar_nsplit)
    bool ln_fold;        // folded LayerNorm (ln_colsum)
    bool per_sample_w;   // per-sample weights (w_sample_stride)
    bool shortcut;       // folded 1x1 shortcut (sc_*)
    bool w_block;        // reads the blocked weight copy (W_blk)
};
const GemmTile* gemm_tile(int cfg);     // nullptr: no such config
// Convolutions whose K steps are whole 64-channel chunks of one source walk K chunk-outer / tap-inner (UNIFORM_TAP of k_gemm and
// k_gemm8): the one predicate, read by both launchers and by the plan query.  p normalised as launch_gemm sees it.
static inline bool gemm_conv_uniform_tap(const GemmParams& p) { return p.Cin % BK == 0 && p.C1 % BK == 0; }
// ring depth and uniform-tap flag of an 8-wave launch (kernels_gemm.hip; p normalised as launch_gemm sees it)
void gemm8_loop_form(const GemmParams& p, int bm, int bn, int splits, int* nst, bool* uni);

// kernels_gemm4s.hip: tile configs 20 - 24
bool gemm4s_supports(const GemmParams& p, int cfg);
int launch_gemm4s(hipStream_t st, const GemmParams& p, int cfg, int splits);

// kernels_gemm_ar.hip: tile config 30, the A-resident kernel for K = 320 / 640 linear problems (declarations the model runtime
// needs are in kernels.h)
bool gemm_ar_supports(const GemmParams& p);
int launch_gemm_ar(hipStream_t st, const GemmParams& p, const void* wpk);
int gemm_ar_nsplit(const GemmParams& p);      // N-range splits per row block = partial sums per row in rowstat_out
bool gemm_sm_supports(const GemmParams& p);    // small-problem kernel (kernels_gemm_sm.hip, tile config 32)
int launch_gemm_sm(hipStream_t st, const GemmParams& p);
