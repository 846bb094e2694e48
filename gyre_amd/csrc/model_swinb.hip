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
// stands beside it and shares only the planner scope and the handle shell.
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

struct gyre_swinb {
    gyre_swinb_cfg cfg;
    Store store;
    Exec ex;
    bool finalized = false;
    float *pe_w = nullptr, *pe_b = nullptr, *pe_g = nullptr, *pe_n = nullptr;
    SwinbStage stage[4];

    void lin(const std::string& key, int O, int I, bool has_bias, UpLin& l) {
        l.K = I; l.N = O;
        l.w = (bf16_t*)store.dmalloc((size_t)O * I * 2, true);
        store.add(key + ".weight", {O, I}, PK_MAT, l.w, O, I);
        if (has_bias) store.vec(key + ".bias", O, &l.b);
    }
    void norm(const std::string& key, int C, float** g, float** b) {
        store.vec(key + ".weight", C, g);
        store.vec(key + ".bias", C, b);
    }
    int build() {
        const gyre_swinb_cfg& c = cfg;
        if (c.window_size != 12) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swinb: window_size 12 is the only one built");
        if (c.ape || !c.patch_norm || !c.qkv_bias) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swinb: ape = False, patch_norm = True, qkv_bias = True is the form built");
        if (c.embed_dim < 32 || c.embed_dim % 32 || c.embed_dim > 256) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swinb: embed_dim must be a multiple of 32, at most 256");
        for (int i = 0; i < 4; ++i) {
            if (c.num_heads[i] != (c.embed_dim / 32) << i) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swinb: head dim 32 with heads doubling per stage is built");
            if (c.depths[i] < 1 || c.depths[i] > 64) GYRE_FAIL(GYRE_ERR_INVALID, "swinb: depth out of range");
        }
        ex.store = &store;
        const int E = c.embed_dim;
        pe_w = (float*)store.dmalloc((size_t)E * 48 * 4, true);
        store.add("patch_embed.proj.weight", {E, 3, 4, 4}, PK_TABLE_F32, pe_w);
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
                b.table = (float*)store.dmalloc((size_t)529 * s.heads * 4, true);
                store.add(p + ".attn.relative_position_bias_table", {529, s.heads}, PK_TABLE_F32, b.table);
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
        for (void* a : store.allocs) if (!a) GYRE_FAIL(GYRE_ERR_HIP, "hipMalloc failed");
        return 0;
    }
    int finalize(hipStream_t st) {
        TRY(store.finalize());
        for (const SwinbStage& s : stage)
            for (const SwinbBlock& b : s.blocks) TRY(launch_win12_bias(st, b.table, s.heads, b.ebias));
        finalized = true;
        return 0;
    }

    // a dry run plans with aligned stand-ins (arena tensors are 256-byte aligned)
    bf16_t* at(const Tn& t) const { return ex.arena.dry ? (bf16_t*)(uintptr_t)4096 : t.p; }
    int linear(const Tn& x, const UpLin& l, const Tn* res, Tn& out) {
        if (x.C != l.K || out.C != l.N || (res && res->C != l.N)) GYRE_FAIL(GYRE_ERR_INVALID, "swinb: internal shape mismatch");
        return ex.linear(at(x), x.C, nullptr, 0, 0, x.rows(), l.K, l.w, l.N, l.b, res ? at(*res) : nullptr, res ? res->C : 0, 0, at(out), out.C);
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
        ex.arena.reset((char*)ws, wsb, dry); ex.st = st; ex.batch = B; ex.cs_unit = 0;
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

extern "C" {

int gyre_swinb_create(const gyre_swinb_cfg* cfg, int device, gyre_swinb** out) { return handle_create(cfg, device, out); }
void gyre_swinb_destroy(gyre_swinb* h) { delete h; }
int gyre_swinb_num_params(const gyre_swinb* h) { return handle_num_params(h); }
const char* gyre_swinb_param_key(const gyre_swinb* h, int i) { return handle_param_key(h, i); }
int gyre_swinb_set_weight(gyre_swinb* h, const char* key, const void* p, int dtype, const int64_t* shape, int ndim, void* st) {
    return handle_set_weight(h, key, p, dtype, shape, ndim, st);
}
int gyre_swinb_finalize(gyre_swinb* h, void* st) {
    if (!h) GYRE_FAIL(GYRE_ERR_INVALID, "null handle");
    return h->finalize((hipStream_t)st);
}
size_t gyre_swinb_workspace_bytes(gyre_swinb* h, int B, int H, int W) { return handle_workspace_bytes(h, B, H, W); }
int gyre_swinb_forward(gyre_swinb* h, void* st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
    return handle_forward(h, "swinb", st, img, idt, B, H, W, ws, wsb, out, odt);
}

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
