// Element-wise kernels of the T2I-adapter graph (model_t2i.hip; reference gyre/pipeline/t2i_adapter/adapter.py): the
// PixelUnshuffle(8) that opens both adapters, the 2x2 average pool of a Downsample without convolution, the ReLU between a block's two
// convolutions, and the NHWC -> NCHW copy that hands a level's feature to the caller.  Everything else of the graph is a convolution
// and runs on the GEMM kernels.  All four are streaming passes with 16-byte accesses on the storage side.
#include "kernels.h"
#include "../../include/gyre_hip.h"

// x NCHW [B][c][H][W] (runtime dtype) -> y NHWC [B][H/8][W/8][64 c], channel = ci * 64 + dy * 8 + dx (torch.nn.PixelUnshuffle(8)).
// One lane per (pixel, ci, dy): the 8 dx values are 8 consecutive input elements and 8 consecutive output channels.
__global__ void k_pixel_unshuffle8(const void* __restrict__ x, int dtype, int c, int H, int W, bf16_t* __restrict__ y, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;        // over B * Ho * Wo * c * 8
    if (i >= total) return;
    const int Ho = H >> 3, Wo = W >> 3;
    const size_t chunk = i % ((size_t)c * 8), pix = i / ((size_t)c * 8);
    const int ci = (int)(chunk >> 3), dy = (int)(chunk & 7);
    const size_t wo = pix % Wo, ho = (pix / Wo) % Ho, b = pix / ((size_t)Wo * Ho);
    const size_t src = ((b * c + ci) * H + ho * 8 + dy) * W + wo * 8;
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = load_as_f32(x, dtype, src + j);
    *(uint4*)(y + i * 8) = pack8(f);
}
int launch_pixel_unshuffle8(hipStream_t st, const void* x, int dtype, int B, int c, int H, int W, bf16_t* y) {
    if (B < 1 || c < 1 || H < 8 || W < 8 || (H & 7) || (W & 7)) GYRE_FAIL(GYRE_ERR_INVALID, "pixel_unshuffle8: H and W must be positive multiples of 8");
    if (dtype < 0 || dtype > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    const size_t total = (size_t)B * (H / 8) * (W / 8) * c * 8;
    hipLaunchKernelGGL(k_pixel_unshuffle8, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, dtype, c, H, W, y, total);
    GYRE_LAUNCH_CHECK();
    return 0;
}

// nn.AvgPool2d(2, 2) over NHWC: y[b][ho][wo][:] = mean of the 2x2 window at (2 ho, 2 wo); an odd last row / column is dropped.
// The four values are summed in fp32 and rounded to storage once.
__global__ void k_avgpool2(const bf16_t* __restrict__ x, int H, int W, int C8, bf16_t* __restrict__ y, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;        // over B * Ho * Wo * C / 8
    if (i >= total) return;
    const int Ho = H >> 1, Wo = W >> 1;
    const size_t c8 = i % C8, pix = i / C8;
    const size_t wo = pix % Wo, ho = (pix / Wo) % Ho, b = pix / ((size_t)Wo * Ho);
    const uint4* r0 = (const uint4*)x + ((b * H + 2 * ho) * W + 2 * wo) * C8 + c8;
    const uint4* r1 = r0 + (size_t)W * C8;
    float a[8], b0[8], c[8], d[8], o[8];
    unpack8(r0[0], a); unpack8(r0[C8], b0); unpack8(r1[0], c); unpack8(r1[C8], d);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = ((a[j] + b0[j]) + (c[j] + d[j])) * 0.25f;
    ((uint4*)y)[i] = pack8(o);
}
int launch_avgpool2(hipStream_t st, const bf16_t* x, int B, int H, int W, int C, bf16_t* y) {
    if (B < 1 || H < 2 || W < 2 || C < 8 || (C & 7)) GYRE_FAIL(GYRE_ERR_INVALID, "avgpool2: H, W >= 2 and C a positive multiple of 8");
    const size_t total = (size_t)B * (H / 2) * (W / 2) * (C / 8);
    hipLaunchKernelGGL(k_avgpool2, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, H, W, C / 8, y, total);
    GYRE_LAUNCH_CHECK();
    return 0;
}

// x = max(x, 0) in place, 8 storage elements per lane.  bf16 and fp16 both carry the sign in bit 15: a negative element becomes +0,
// except a NaN, which stays a NaN whatever its sign (torch.relu propagates it; magnitude bits above the infinity pattern).
__global__ void k_relu(uint4* __restrict__ x, size_t n8) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    uint4 v = x[i];
    auto keep = [](uint32_t h) -> bool { return !(h & 0x8000u) || (h & 0x7fffu) > GYRE_INF_BITS; };
    auto r = [&](uint32_t w) -> uint32_t { return w & ((keep(w & 0xffffu) ? 0xffffu : 0u) | (keep(w >> 16) ? 0xffff0000u : 0u)); };
    v.x = r(v.x); v.y = r(v.y); v.z = r(v.z); v.w = r(v.w);
    x[i] = v;
}
int launch_relu(hipStream_t st, bf16_t* x, size_t n) {
    if (n == 0 || (n & 7)) GYRE_FAIL(GYRE_ERR_INVALID, "relu: the element count must be a positive multiple of 8");
    hipLaunchKernelGGL(k_relu, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, st, (uint4*)x, n / 8);
    GYRE_LAUNCH_CHECK();
    return 0;
}

// y NCHW [B][C][HW] (runtime dtype) = x NHWC [B][HW][Cpad], the first C channels
__global__ void k_nhwc_to_nchw_any(const bf16_t* __restrict__ x, int C, int HW, int Cpad, void* __restrict__ y, int dtype, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;        // over B * C * HW (output order)
    if (i >= total) return;
    const size_t p = i % HW, c = (i / HW) % C, n = i / ((size_t)HW * C);
    store_from_f32(y, dtype, i, bf16_to_f32(x[(n * HW + p) * Cpad + c]));
}
int launch_nhwc_to_nchw(hipStream_t st, const bf16_t* x, int B, int C, int HW, int Cpad, void* y, int dtype) {
    if (dtype < 0 || dtype > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    const size_t total = (size_t)B * C * HW;
    hipLaunchKernelGGL(k_nhwc_to_nchw_any, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, C, HW, Cpad, y, dtype, total);
    GYRE_LAUNCH_CHECK();
    return 0;
}
