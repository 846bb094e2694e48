// Element-wise kernels of the ControlNet graph (model_ctrl.hip): the SiLU between the convolutions of the hint-image embedding (the
// library has SiLU only fused into GroupNorm) and the hand-off of one zero-convolution output to the UNet's residual inputs - a scaled,
// optionally accumulating, optionally masked NHWC -> NCHW copy into a batch window of the caller's buffer.  Everything else of the graph runs on the
// kernels the UNet already uses.  Both are streaming passes with 16-byte accesses on the storage side.
#include "kernels.h"
#include "../../include/gyre_hip.h"

// x = x * sigmoid(x) in place, 8 storage elements per lane: fp32 math (silu_f: exp2 and the hardware reciprocal), one rounding to storage.
// NaN stays NaN; a large negative x goes to -0 through the overflow of the exponential (rcp(inf) = 0), never through inf * 0.
__global__ void k_silu(uint4* __restrict__ x, size_t n8) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    float f[8];
    unpack8(x[i], f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = silu_f(f[j]);
    x[i] = pack8(f);
}
int launch_silu(hipStream_t st, bf16_t* x, size_t n) {
    if (n == 0 || (n & 7)) GYRE_FAIL(GYRE_ERR_INVALID, "silu: the element count must be a positive multiple of 8");
    hipLaunchKernelGGL(k_silu, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, st, (uint4*)x, n / 8);
    GYRE_LAUNCH_CHECK();
    return 0;
}

// One workgroup moves a tile of 64 pixels x 64 channels of one output sample.
//   load : lane = (pixel, 8-channel chunk), one 16-byte read along C, written to the LDS tile as four dwords
//   store: lane = pixel, wave = 16 channels; a wave writes 64 consecutive pixels of one channel row (256 B of fp32)
// The tile is [64 pixels][32 dwords + 1]: with the odd row stride both sides are free of bank conflicts - the writers of a 32-lane group
// (4 pixels x 8 chunks) hit dword 33 p + 4 chunk + k, the readers (32 pixels, one channel pair) 33 p + c / 2.
// A sample of `out` outside [b0, b0 + B) is written as zeros (assign mode only; the grid of an accumulate call does not cover it).
#define CE_TP 64
#define CE_TC 64
#define CE_LD (CE_TC / 2 + 1)
// MASKED: the store-phase lane (one pixel) reads m = mask[mb][p] once - a wave reads 64 consecutive floats, 256 B - and reuses it for
// its 16 channels: out = rnd(fl(fl(scale f) m) [+ old]).  m == 0 gives +-0 for a finite f, NaN stays NaN.  The unmasked instantiation
// is the kernel as it was: no mask argument is read and no instruction is added.
template <bool MASKED>
__device__ __forceinline__ void ctrl_emit_body(const bf16_t* __restrict__ f, int B, int C, int HW, int Cpad, float scale, int accumulate,
                                               void* __restrict__ out, int dtype, int b0, const float* __restrict__ mask, int mask_B) {
    __shared__ uint32_t tile[CE_TP * CE_LD];
    const int tid = threadIdx.x;
    const int p0 = blockIdx.x * CE_TP, c0 = blockIdx.y * CE_TC;
    const int ob = accumulate ? b0 + (int)blockIdx.z : (int)blockIdx.z;      // sample of `out`
    const int b = ob - b0;                                                    // sample of f
    const bool live = b >= 0 && b < B;                                        // (uniform over the workgroup)
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int q = tid + r * 256, chunk = q & 7, pl = q >> 3;
        uint4 v = {0u, 0u, 0u, 0u};
        const int p = p0 + pl, c = c0 + chunk * 8;
        if (live && p < HW && c < Cpad) v = *(const uint4*)(f + ((size_t)b * HW + p) * Cpad + c);
        uint32_t* t = tile + pl * CE_LD + chunk * 4;
        t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
    }
    __syncthreads();
    const int pl = tid & 63, cw = (tid >> 6) * 16, p = p0 + pl;
    if (p >= HW) return;
    float m = 1.f;
    if (MASKED) m = live ? mask[(size_t)(mask_B == 1 ? 0 : b) * HW + p] : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t w = tile[pl * CE_LD + (cw >> 1) + j];
        const float v2[2] = {bf16lo(w), bf16hi(w)};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = c0 + cw + 2 * j + h;
            if (c >= C) continue;
            const size_t o = ((size_t)ob * C + c) * HW + p;
            float val = live ? __fmul_rn(scale, v2[h]) : 0.f;
            if (MASKED) val = live ? __fmul_rn(val, m) : 0.f;
            if (accumulate) val = __fadd_rn(load_as_f32(out, dtype, o), val);
            store_from_f32(out, dtype, o, val);
        }
    }
}
__global__ __launch_bounds__(256) void k_ctrl_emit(const bf16_t* __restrict__ f, int B, int C, int HW, int Cpad, float scale, int accumulate,
                                                   void* __restrict__ out, int dtype, int b0) {
    ctrl_emit_body<false>(f, B, C, HW, Cpad, scale, accumulate, out, dtype, b0, nullptr, 0);
}
__global__ __launch_bounds__(256) void k_ctrl_emit_masked(const bf16_t* __restrict__ f, int B, int C, int HW, int Cpad, float scale,
                                                          int accumulate, void* __restrict__ out, int dtype, int b0,
                                                          const float* __restrict__ mask, int mask_B) {
    ctrl_emit_body<true>(f, B, C, HW, Cpad, scale, accumulate, out, dtype, b0, mask, mask_B);
}
// mask == nullptr: the unmasked kernel; otherwise fp32 [mask_B][HW] with mask_B == 1 (one mask for every sample) or B
int launch_ctrl_emit_masked(hipStream_t st, const bf16_t* f, int B, int C, int HW, int Cpad, float scale, int accumulate, void* out,
                            int out_dtype, int out_B, int out_b0, const float* mask, int mask_B) {
    if (out_dtype < 0 || out_dtype > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    if (B < 1 || C < 1 || HW < 1 || Cpad < C || (Cpad & 7)) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl_emit: needs B, C, HW >= 1 and Cpad >= C a multiple of 8");
    if (out_b0 < 0 || out_B < 1 || out_b0 + B > out_B) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl_emit: the samples [out_b0, out_b0 + B) must lie inside the output batch");
    if (mask && mask_B != 1 && mask_B != B) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl_emit: the mask needs batch 1 or B");
    const int nz = accumulate ? B : out_B;
    if (nz > 65535 || (C + CE_TC - 1) / CE_TC > 65535) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl_emit: batch or channel count beyond the grid");
    const dim3 grid((unsigned)((HW + CE_TP - 1) / CE_TP), (unsigned)((C + CE_TC - 1) / CE_TC), (unsigned)nz);
    if (mask)
        hipLaunchKernelGGL(k_ctrl_emit_masked, grid, dim3(256), 0, st, f, B, C, HW, Cpad, scale, accumulate ? 1 : 0, out, out_dtype, out_b0,
                           mask, mask_B);
    else
        hipLaunchKernelGGL(k_ctrl_emit, grid, dim3(256), 0, st, f, B, C, HW, Cpad, scale, accumulate ? 1 : 0, out, out_dtype, out_b0);
    GYRE_LAUNCH_CHECK();
    return 0;
}
int launch_ctrl_emit(hipStream_t st, const bf16_t* f, int B, int C, int HW, int Cpad, float scale, int accumulate, void* out,
                     int out_dtype, int out_B, int out_b0) {
    return launch_ctrl_emit_masked(st, f, B, C, HW, Cpad, scale, accumulate, out, out_dtype, out_B, out_b0, nullptr, 0);
}
