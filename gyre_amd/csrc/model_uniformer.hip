// The UniFormer backbone of the segmentation annotator and its C ABI (include/gyre_hip.h): the reference's UniFormer (gyre/pipeline/
// hinters/models/uniformer.py) with global attention in stages 3 and 4 (windows = False, hybrid = False), head dim 64, which the mmseg
// UPerNet head of the hinters-uniformer engine takes as its backbone.  The head stays a host module.
//
// Topology, every activation NHWC [B][h][w][C] in the storage type, C = embed_dim[stage] (multiples of 64: no padding channels):
//   embed S   space-to-depth gather (k_uf_gather_img for the 4 x 4 / stride 4 embedding of the NCHW image, 3 channels at a pitch of 4:
//             K = 64; k_uf_gather for the 2 x 2 / stride 2 ones, K = 4 C) -> the convolution as a planner GEMM on weights repacked
//             to the gather's column order at load (PK_CONV_PATCH) -> patch_embedS.norm (eps 1e-5).  Floor division: a trailing odd
//             row / column is dropped as the unpadded convolution drops it.
//   CBlock    (stages 1, 2)  u = x + dw3x3(x) (k_uf_cpe);  v = u + conv2(dw5x5(conv1(BN1(u)))) - ONE launch of k_uf_local<C>, BN1 folded
//             into conv1;  x' = v + fc2(gelu(fc1(BN2(v)))) - two planner GEMMs, BN2 folded into fc1, the erf GELU the in-place
//             launch_swin_act, the residual in fc2's epilogue.
//   SABlock   (stages 3, 4)  u = x + dw3x3(x);  y = u + proj(attention(qkv(LN1(u))));  x' = y + fc2(gelu(fc1(LN2(y)))), LayerNorm eps
//             1e-6.  q | k are one GEMM on the first 2 C rows of attn.qkv (nn.Linear's [3][heads][64] column order is the attention
//             kernel's layout), V^T a second one through the transposing epilogue on the last C rows - the pair the UNet runs when the
//             fused q | k + V^T tile condition does not hold, which the biased projection rules out here; launch_attention at D = 64
//             over all h w tokens of the sample (the softmax scale is applied to the fp32 logits).
//   stage out normS (eps 1e-6) -> launch_nhwc_to_nchw into the caller's buffer: map S
//
// finalize folds each BatchNorm into the 1x1 convolution it feeds (launch_uf_fold: fp32 from fp32 staging copies of the raw parameters,
// one rounding to storage; exact, since the norm feeds the convolution directly) and transposes the depthwise weights to [taps][C] fp32.
// The planner sees every launch as if its sample ran alone (BatchInvariantScope); the other kernels work per pixel, tile or sample.
// The weight registration, the planner calls with their shape checks and the C ABI shell are ImageGraph's (model_upscaler.h).
#include "model_upscaler.h"

namespace {
struct UfBlock {
    float *pe_raw, *pe_b, *pe_w;                           // pos_embed [C][1][3][3] staged, its bias, [9][C]
    // CBlock
    Bn bn1, bn2;
    float *c1_raw, *c1_b, *b1f, *dw_raw, *dw_b, *dw_w, *f1_raw, *f1_b;
    bf16_t* w1f;
    UpLin conv2;
    // SABlock
    float *g1, *b1, *g2, *b2;
    UpLin qkv, proj;
    // both (a CBlock's fc1 holds the folded copy)
    UpLin fc1, fc2;
};
struct UfStage {
    int C = 0, heads = 0, patch = 2, Kin = 0;
    UpLin pe; float *pe_g = nullptr, *pe_b = nullptr;      // patch_embedS.proj, .norm
    std::vector<UfBlock> blocks;
    float *ng = nullptr, *nb = nullptr;                    // normS
};
}  // namespace

struct gyre_uniformer : ImageGraph {
    gyre_uniformer_cfg cfg;
    UfStage stage[4];
    gyre_uniformer() : ImageGraph("uniformer") {}

    // no padding anywhere (every width is a multiple of 64), a bias everywhere
    void lin(const std::string& key, int O, int I, bool conv1x1, UpLin& l) { ImageGraph::lin(key, O, I, O, I, true, conv1x1, l); }
    void pos_embed(const std::string& p, int C, UfBlock& b) {
        b.pe_raw = f32(p + ".pos_embed.weight", {C, 1, 3, 3});
        store.vec(p + ".pos_embed.bias", C, &b.pe_b);
        b.pe_w = (float*)store.dmalloc((size_t)9 * C * 4, false);
    }
    int build() {
        const gyre_uniformer_cfg& c = cfg;
        if (c.windows || c.hybrid) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "uniformer: global attention in stage 3 (windows = False, hybrid = False) is the form built");
        if (c.head_dim != 64 || c.mlp_ratio != 4 || !c.qkv_bias) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "uniformer: head_dim 64, mlp_ratio 4, qkv_bias = True is the form built");
        if (c.embed_dim[0] != 64 || c.embed_dim[1] != 128) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "uniformer: the local-relation kernel is built for embed_dim[0:2] = (64, 128)");
        for (int i = 0; i < 4; ++i) {
            if (c.embed_dim[i] < 64 || c.embed_dim[i] % 64 || c.embed_dim[i] > 1024) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "uniformer: widths must be multiples of 64, at most 1024");
            if (c.layers[i] < 1 || c.layers[i] > 64) GYRE_FAIL(GYRE_ERR_INVALID, "uniformer: 1 to 64 blocks per stage");
        }
        for (int i = 0; i < 4; ++i) {
            UfStage& s = stage[i];
            s.C = c.embed_dim[i]; s.heads = s.C / 64; s.patch = i ? 2 : 4;
            const int cin = i ? c.embed_dim[i - 1] : 3, cpad = i ? cin : 4;
            s.Kin = s.patch * s.patch * cpad;
            const std::string p = "patch_embed" + std::to_string(i + 1);
            norm(p + ".norm", s.C, &s.pe_g, &s.pe_b);
            s.pe.K = s.Kin; s.pe.N = s.C;
            s.pe.w = (bf16_t*)store.dmalloc((size_t)s.C * s.Kin * 2, true);
            store.add(p + ".proj.weight", {s.C, cin, s.patch, s.patch}, PK_CONV_PATCH, s.pe.w, s.C, cpad);
            store.vec(p + ".proj.bias", s.C, &s.pe.b);
        }
        for (int i = 0; i < 4; ++i) {
            UfStage& s = stage[i];
            const int C = s.C;
            for (int j = 0; j < c.layers[i]; ++j) {
                const std::string p = "blocks" + std::to_string(i + 1) + "." + std::to_string(j);
                UfBlock b = {};
                pos_embed(p, C, b);
                if (i < 2) {
                    bnorm(p + ".norm1", C, b.bn1);
                    b.c1_raw = f32(p + ".conv1.weight", {C, C, 1, 1});
                    store.vec(p + ".conv1.bias", C, &b.c1_b);
                    b.w1f = (bf16_t*)store.dmalloc((size_t)C * C * 2, false);
                    b.b1f = (float*)store.dmalloc((size_t)C * 4, false);
                    lin(p + ".conv2", C, C, true, b.conv2);
                    b.dw_raw = f32(p + ".attn.weight", {C, 1, 5, 5});
                    store.vec(p + ".attn.bias", C, &b.dw_b);
                    b.dw_w = (float*)store.dmalloc((size_t)25 * C * 4, false);
                    bnorm(p + ".norm2", C, b.bn2);
                    b.f1_raw = f32(p + ".mlp.fc1.weight", {4 * C, C, 1, 1});
                    store.vec(p + ".mlp.fc1.bias", 4 * C, &b.f1_b);
                    b.fc1.K = C; b.fc1.N = 4 * C;
                    b.fc1.w = (bf16_t*)store.dmalloc((size_t)4 * C * C * 2, false);
                    b.fc1.b = (float*)store.dmalloc((size_t)4 * C * 4, false);
                    lin(p + ".mlp.fc2", C, 4 * C, true, b.fc2);
                } else {
                    norm(p + ".norm1", C, &b.g1, &b.b1);
                    lin(p + ".attn.qkv", 3 * C, C, false, b.qkv);
                    lin(p + ".attn.proj", C, C, false, b.proj);
                    norm(p + ".norm2", C, &b.g2, &b.b2);
                    lin(p + ".mlp.fc1", 4 * C, C, false, b.fc1);
                    lin(p + ".mlp.fc2", C, 4 * C, false, b.fc2);
                }
                s.blocks.push_back(b);
            }
            norm("norm" + std::to_string(i + 1), C, &s.ng, &s.nb);
        }
        return check_allocs();
    }
    int finalize(hipStream_t st) {
        TRY(store.finalize());
        for (int i = 0; i < 4; ++i) {
            const int C = stage[i].C;
            for (const UfBlock& b : stage[i].blocks) {
                TRY(launch_uf_taps(st, b.pe_raw, C, 9, b.pe_w));
                if (i >= 2) continue;
                TRY(launch_uf_fold(st, b.c1_raw, b.c1_b, b.bn1.g, b.bn1.b, b.bn1.m, b.bn1.v, 1e-5f, C, C, b.w1f, b.b1f));
                TRY(launch_uf_taps(st, b.dw_raw, C, 25, b.dw_w));
                TRY(launch_uf_fold(st, b.f1_raw, b.f1_b, b.bn2.g, b.bn2.b, b.bn2.m, b.bn2.v, 1e-5f, 4 * C, C, b.fc1.w, b.fc1.b));
            }
        }
        finalized = true;
        return 0;
    }

    int ln(const Tn& x, const float* g, const float* b, float eps, Tn& y) {
        if (ex.dry()) return 0;
        return launch_layernorm(ex.st, x.p, x.rows(), x.C, g, b, eps, y.p);
    }
    // x' = v + fc2(gelu(fc1(src))), src = v (CBlock: BN2 is inside fc1) or LN2(v)
    int mlp(const UfBlock& b, const Tn& src, const Tn& v, Tn& hdn, Tn& out) {
        TRY(linear(src, b.fc1, nullptr, hdn));
        if (!ex.dry()) TRY(launch_swin_act(ex.st, hdn.p, (size_t)hdn.rows() * hdn.C, 0, 0.f));
        return linear(hdn, b.fc2, &v, out);
    }

    int run(bool dry, hipStream_t st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
        if (B < 1 || B > 65535) GYRE_FAIL(GYRE_ERR_INVALID, "uniformer: a batch of 1 to 65535");
        if (H < 32 || W < 32) GYRE_FAIL(GYRE_ERR_INVALID, "uniformer: H and W must be at least 32, got " + std::to_string(H) + " x " + std::to_string(W));
        int h = H / 4, w = W / 4;
        // the planner indexes rows with 32-bit integers; the widest row is the MLP's 4 C (the maps shrink 4 x per stage, C at most 2 x .. 8 x)
        for (int i = 0; i < 4; ++i)
            if ((size_t)B * (h >> i) * (w >> i) > 0x3fffffff / (4 * (size_t)stage[i].C)) GYRE_FAIL(GYRE_ERR_INVALID, "uniformer: image too large");
        if (!dry && !out) GYRE_FAIL(GYRE_ERR_INVALID, "uniformer: null output buffer");
        BatchInvariantScope invariant;
        begin(dry, st, B, ws, wsb);
        const size_t osz = odt == 0 ? 4 : 2;
        char* op = (char*)out;
        Tn a;                                                                 // the residual stream of the stage
        for (int i = 0; i < 4; ++i) {
            const UfStage& s = stage[i];
            const int C = s.C;
            {   // patch embedding: gather -> GEMM -> LayerNorm
                Tn g, e;
                if (i) { h /= 2; w /= 2; }
                TRY(ex.alloc(g, B, h, w, s.Kin));
                if (!dry) {
                    if (i) TRY(launch_uf_gather(st, a.p, B, a.H, a.W, a.C, g.p));
                    else TRY(launch_uf_gather_img(st, img, idt, B, H, W, g.p));
                }
                if (i) ex.free(a);
                TRY(ex.alloc(e, B, h, w, C));
                TRY(linear(g, s.pe, nullptr, e));
                ex.free(g);
                TRY(ex.alloc(a, B, h, w, C));
                TRY(ln(e, s.pe_g, s.pe_b, 1e-5f, a));
                ex.free(e);
            }
            Tn u, v, hdn, nrm, qk, vt, ao;
            const int N = h * w, ldvt = (N + 7) / 8 * 8;
            TRY(ex.alloc(u, B, h, w, C));
            TRY(ex.alloc(v, B, h, w, C));
            TRY(ex.alloc(hdn, B, h, w, 4 * C));
            TRY(ex.alloc(nrm, B, h, w, C));
            if (i >= 2) {
                TRY(ex.alloc(qk, B, h, w, 2 * C));
                TRY(ex.alloc(vt, B, C, 1, ldvt));
                TRY(ex.alloc(ao, B, h, w, C));
            }
            for (const UfBlock& b : s.blocks) {
                if (!dry) TRY(launch_uf_cpe(st, a.p, B, h, w, C, b.pe_w, b.pe_b, u.p));
                if (i < 2) {
                    if (!dry) TRY(launch_uf_local(st, u.p, C, v.p, C, B, h, w, C, b.w1f, b.b1f, b.dw_w, b.dw_b, b.conv2.w, b.conv2.b));
                    TRY(mlp(b, v, v, hdn, a));
                } else {
                    TRY(ln(u, b.g1, b.b1, 1e-6f, nrm));
                    TRY(linear_to(nrm, b.qkv.w, b.qkv.b, C, 2 * C, nullptr, at(qk), 2 * C));
                    TRY(ex.linear_t(nrm.p, C, B * N, C, b.qkv.w + (size_t)2 * C * C, C, b.qkv.b + 2 * C, N, ldvt, vt.p));
                    if (!dry) {
                        AttnParams ap;
                        ap.q = qk.p; ap.ldq = 2 * C; ap.k = qk.p + C; ap.ldk = 2 * C; ap.vt = vt.p; ap.ldvt = ldvt; ap.o = ao.p; ap.ldo = C;
                        ap.B = B; ap.H = s.heads; ap.Nq = N; ap.Nk = N; ap.D = 64; ap.k_prescaled = 0;
                        TRY(launch_attention(st, ap));
                    }
                    TRY(linear(ao, b.proj, &u, v));
                    TRY(ln(v, b.g2, b.b2, 1e-6f, nrm));
                    TRY(mlp(b, nrm, v, hdn, a));
                }
            }
            ex.free(qk); ex.free(vt); ex.free(ao); ex.free(hdn); ex.free(u); ex.free(v);
            TRY(ln(a, s.ng, s.nb, 1e-6f, nrm));
            if (!dry) TRY(launch_nhwc_to_nchw(st, nrm.p, B, C, N, C, op, odt));
            op += (size_t)B * C * N * osz;
            ex.free(nrm);
        }
        ex.free(a);
        return 0;
    }
};

GYRE_IMAGE_MODEL_ABI(uniformer)

extern "C" {


// ---- test hooks of kernels_uniformer.hip ----
int gyre_op_uf_local(void* st, const void* x, int ldx, void* y, int ldy, int B, int H, int W, int C, const void* w1, const float* b1,
                     const float* wd, const float* bd, const void* w2, const float* b2) {
    return launch_uf_local((hipStream_t)st, (const bf16_t*)x, ldx, (bf16_t*)y, ldy, B, H, W, C, (const bf16_t*)w1, b1, wd, bd, (const bf16_t*)w2, b2);
}
int gyre_op_uf_local_tile(int32_t* rows, int32_t* cols) {
    if (!rows || !cols) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    int th, tw;
    uf_local_tile(&th, &tw);
    *rows = th; *cols = tw;
    return 0;
}
int gyre_op_uf_cpe(void* st, const void* x, int B, int H, int W, int C, const float* w, const float* bias, void* y) {
    return launch_uf_cpe((hipStream_t)st, (const bf16_t*)x, B, H, W, C, w, bias, (bf16_t*)y);
}
int gyre_op_uf_gather(void* st, const void* x, int B, int H, int W, int C, void* y) {
    return launch_uf_gather((hipStream_t)st, (const bf16_t*)x, B, H, W, C, (bf16_t*)y);
}
int gyre_op_uf_gather_img(void* st, const void* x, int dtype, int B, int H, int W, void* y) {
    return launch_uf_gather_img((hipStream_t)st, x, dtype, B, H, W, (bf16_t*)y);
}
int gyre_op_uf_fold(void* st, const float* w, const float* b, const float* gamma, const float* beta, const float* mean, const float* var,
                    float eps, int O, int I, void* wout, float* bout) {
    return launch_uf_fold((hipStream_t)st, w, b, gamma, beta, mean, var, eps, O, I, (bf16_t*)wout, bout);
}
int gyre_op_uf_taps(void* st, const float* w, int C, int T, float* out) { return launch_uf_taps((hipStream_t)st, w, C, T, out); }

}  // extern "C"
