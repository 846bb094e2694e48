// The Swin-B backbone of InSPyReNet and its C ABI (include/gyre_hip.h): the reference's SwinTransformer (gyre/pipeline/hinters/inspyrenet/
// backbones/SwinTransformer.py) as SwinB() builds it - window 12, head dim 32, heads doubling per stage - which InSPyReNet takes as a module.
//
// Topology, every activation in token order [B][h][w][C] in the storage type, C = embed_dim 2^stage (a multiple of 32: no padding channels):
//   embed     k_swinb_embed: 4x4 / stride 4 convolution of the zero-padded image + patch_embed.norm -> tokens at h0 = ceil(H / 4); map 0
//   block     y = x + proj(win12_attn(qkv(norm1(x))));  x' = y + fc2(gelu(fc1(norm2(y)))), shift 6 in every odd block (BasicLayer passes
//             window_size // 2 whatever the map size).  qkv, proj, fc1, fc2 run on the planner, the residuals in their epilogues; the
//             norms are launch_layernorm, the erf GELU the in-place launch_swin_act.  nn.Linear's qkv column order [3][heads][32] IS
//             the kernel's layout at head dim 32, so the weights load as plain matrices; the padded map, the roll and the window
//             partition exist only as the index map of k_win12_attn, which also stands the qkv bias in for the padded tokens.
//   stage out norm_i -> launch_nhwc_to_nchw into the caller's buffer: map i + 1
//   merge     k_swinb_merge_ln (2 x 2 gather + LayerNorm over 4 C, written once) -> the bias-free 4 C -> 2 C reduction on the planner
// The model_upscaler.h trunk does not fit (head dim 30 at a 32 pitch, padded widths, conv_first, one width for all layers), so this graph
// stands beside it on the same base, ImageGraph: the weight registration, the planner linear, the dry-run pointer and the C ABI shell.
//
// finalize expands every block's relative-position table into the register order of k_win12_attn (launch_win12_bias), 81 KB per head.
// The planner sees every launch as if its sample ran alone (BatchInvariantScope); the other kernels work per token or per window.
#include "model_upscaler.h"

namespace {
struct SwinbBlock { float *g1, *b1, *g2, *b2, *table, *ebias; UpLin qkv, proj, fc1, fc2; int shift; };
struct SwinbStage {
    int C = 0, heads = 0;
    std::vector<SwinbBlock> blocks;
    float *ng = nullptr, *nb = nullptr;                  // norm{i}
    float *mg = nullptr, *mb = nullptr; UpLin red;       // downsample.norm, downsample.reduction (stages 0 .. 2)
};
}  // namespace

struct gyre_swinb : ImageGraph {
    gyre_swinb_cfg cfg;
    float *pe_w = nullptr, *pe_b = nullptr, *pe_g = nullptr, *pe_n = nullptr;
    SwinbStage stage[4];
    gyre_swinb() : ImageGraph("swinb") {}

    // no padding anywhere: every width is a multiple of 32
    void lin(const std::string& key, int O, int I, bool has_bias, UpLin& l) { ImageGraph::lin(key, O, I, O, I, has_bias, false, l); }
    int build() {
        const gyre_swinb_cfg& c = cfg;
        if (c.window_size != 12) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swinb: window_size 12 is the only one built");
        if (c.ape || !c.patch_norm || !c.qkv_bias) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swinb: ape = False, patch_norm = True, qkv_bias = True is the form built");
        if (c.embed_dim < 32 || c.embed_dim % 32 || c.embed_dim > 256) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swinb: embed_dim must be a multiple of 32, at most 256");
        for (int i = 0; i < 4; ++i) {
            if (c.num_heads[i] != (c.embed_dim / 32) << i) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swinb: head dim 32 with heads doubling per stage is built");
            if (c.depths[i] < 1 || c.depths[i] > 64) GYRE_FAIL(GYRE_ERR_INVALID, "swinb: depth out of range");
        }
        const int E = c.embed_dim;
        pe_w = f32("patch_embed.proj.weight", {E, 3, 4, 4});
        store.vec("patch_embed.proj.bias", E, &pe_b);
        norm("patch_embed.norm", E, &pe_g, &pe_n);
        for (int i = 0; i < 4; ++i) {
            SwinbStage& s = stage[i];
            s.C = E << i; s.heads = c.num_heads[i];
            for (int j = 0; j < c.depths[i]; ++j) {
                const std::string p = "layers." + std::to_string(i) + ".blocks." + std::to_string(j);
                SwinbBlock b;
                b.shift = (j & 1) ? 6 : 0;
                norm(p + ".norm1", s.C, &b.g1, &b.b1);
                b.table = f32(p + ".attn.relative_position_bias_table", {529, s.heads});
                b.ebias = (float*)store.dmalloc((size_t)s.heads * 144 * 144 * 4, false);
                lin(p + ".attn.qkv", 3 * s.C, s.C, true, b.qkv);
                lin(p + ".attn.proj", s.C, s.C, true, b.proj);
                norm(p + ".norm2", s.C, &b.g2, &b.b2);
                lin(p + ".mlp.fc1", 4 * s.C, s.C, true, b.fc1);
                lin(p + ".mlp.fc2", s.C, 4 * s.C, true, b.fc2);
                s.blocks.push_back(b);
            }
            if (i < 3) {
                const std::string p = "layers." + std::to_string(i) + ".downsample";
                lin(p + ".reduction", 2 * s.C, 4 * s.C, false, s.red);
                norm(p + ".norm", 4 * s.C, &s.mg, &s.mb);
            }
        }
        for (int i = 0; i < 4; ++i) norm("norm" + std::to_string(i), stage[i].C, &stage[i].ng, &stage[i].nb);
        return check_allocs();
    }
    int finalize(hipStream_t st) {
        TRY(store.finalize());
        for (const SwinbStage& s : stage)
            for (const SwinbBlock& b : s.blocks) TRY(launch_win12_bias(st, b.table, s.heads, b.ebias));
        finalized = true;
        return 0;
    }

    int ln(const Tn& x, const float* g, const float* b, Tn& y) {
        if (ex.dry()) return 0;
        return launch_layernorm(ex.st, x.p, x.rows(), x.C, g, b, 1e-5f, y.p);
    }

    int run(bool dry, hipStream_t st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
        if (B < 1 || B > 65535) GYRE_FAIL(GYRE_ERR_INVALID, "swinb: a batch of 1 to 65535");
        if (H < 4 || W < 4) GYRE_FAIL(GYRE_ERR_INVALID, "swinb: H and W must be at least 4, got " + std::to_string(H) + " x " + std::to_string(W));
        int h = (H + 3) / 4, w = (W + 3) / 4;
        // the planner indexes rows with 32-bit integers; the widest row is the MLP's 4 C
        if ((size_t)B * h * w > 0x3fffffff / (4 * (size_t)cfg.embed_dim)) GYRE_FAIL(GYRE_ERR_INVALID, "swinb: image too large");
        if (!dry && !out) GYRE_FAIL(GYRE_ERR_INVALID, "swinb: null output buffer");
        BatchInvariantScope invariant;
        begin(dry, st, B, ws, wsb);
        const size_t osz = odt == 0 ? 4 : 2;
        char* op = (char*)out;
        Tn a;
        TRY(ex.alloc(a, B, h, w, cfg.embed_dim));
        if (!dry) {
            TRY(launch_swinb_embed(st, img, idt, B, H, W, cfg.embed_dim, pe_w, pe_b, pe_g, pe_n, 1e-5f, a.p));
            TRY(launch_nhwc_to_nchw(st, a.p, B, a.C, h * w, a.C, op, odt));
        }
        op += (size_t)B * a.C * h * w * osz;
        for (int i = 0; i < 4; ++i) {
            const SwinbStage& s = stage[i];
            const int C = s.C;
            Tn u, nrm, qkv, ao, hdn;
            TRY(ex.alloc(u, B, h, w, C));
            TRY(ex.alloc(nrm, B, h, w, C));
            TRY(ex.alloc(qkv, B, h, w, 3 * C));
            TRY(ex.alloc(ao, B, h, w, C));
            TRY(ex.alloc(hdn, B, h, w, 4 * C));
            for (const SwinbBlock& b : s.blocks) {
                TRY(ln(a, b.g1, b.b1, nrm));
                TRY(linear(nrm, b.qkv, nullptr, qkv));
                if (!dry) TRY(launch_win12_attn(st, qkv.p, qkv.C, b.qkv.b, ao.p, ao.C, b.ebias, B, h, w, s.heads, b.shift));
                TRY(linear(ao, b.proj, &a, u));                                   // y = x + proj(attn)
                TRY(ln(u, b.g2, b.b2, nrm));
                TRY(linear(nrm, b.fc1, nullptr, hdn));
                if (!dry) TRY(launch_swin_act(st, hdn.p, (size_t)hdn.rows() * hdn.C, 0, 0.f));
                TRY(linear(hdn, b.fc2, &u, a));                                   // x' = y + fc2(gelu(fc1(norm2(y))))
            }
            ex.free(qkv); ex.free(ao); ex.free(hdn); ex.free(u);
            TRY(ln(a, s.ng, s.nb, nrm));
            if (!dry) TRY(launch_nhwc_to_nchw(st, nrm.p, B, C, h * w, C, op, odt));
            op += (size_t)B * C * h * w * osz;
            ex.free(nrm);
            if (i < 3) {
                const int h2 = (h + 1) / 2, w2 = (w + 1) / 2;
                Tn m, nx;
                TRY(ex.alloc(m, B, h2, w2, 4 * C));
                if (!dry) TRY(launch_swinb_merge_ln(st, a.p, B, h, w, C, s.mg, s.mb, 1e-5f, m.p));
                ex.free(a);
                TRY(ex.alloc(nx, B, h2, w2, 2 * C));
                TRY(linear(m, s.red, nullptr, nx));
                ex.free(m);
                a = nx; h = h2; w = w2;
            }
        }
        ex.free(a);
        return 0;
    }
};

GYRE_IMAGE_MODEL_ABI(swinb)

extern "C" {


// ---- test hooks of kernels_swinb.hip ----
int gyre_op_win12_bias(void* st, const float* table, int heads, float* out) { return launch_win12_bias((hipStream_t)st, table, heads, out); }
int gyre_op_win12_attn(void* st, const void* qkv, int ld_qkv, const float* qkv_bias, void* o, int ld_o, const float* bias, int B, int H, int W,
                       int heads, int shift) {
    return launch_win12_attn((hipStream_t)st, (const bf16_t*)qkv, ld_qkv, qkv_bias, (bf16_t*)o, ld_o, bias, B, H, W, heads, shift);
}
int gyre_op_swinb_embed(void* st, const void* x, int dtype, int B, int H, int W, int C, const float* w, const float* bias, const float* gamma,
                        const float* beta, void* y) {
    return launch_swinb_embed((hipStream_t)st, x, dtype, B, H, W, C, w, bias, gamma, beta, 1e-5f, (bf16_t*)y);
}
int gyre_op_swinb_merge_ln(void* st, const void* x, int B, int H, int W, int C, const float* gamma, const float* beta, void* y) {
    return launch_swinb_merge_ln((hipStream_t)st, (const bf16_t*)x, B, H, W, C, gamma, beta, 1e-5f, (bf16_t*)y);
}

}  // extern "C"
