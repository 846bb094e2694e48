// SwinIR upscaler graph and its C ABI (include/gyre_hip.h).
//
// Topology restates the reference's vendored model (gyre/pipeline/upscalers/models/network_swinir.py, SwinIR.forward with
// upsampler == "nearest+conv", lines 810-845; the block: SwinTransformerBlock.forward 244-284, the RSTB: 486-487):
//   (x - mean) * img_range, conv_first, patch_embed.norm, per RSTB: blocks, then conv (1conv / 3conv) + the RSTB input,
//   norm, conv_after_body + conv_first's output, lrelu_0.01(conv_before_upsample), lrelu(conv_up1(nearest 2x)),
//   lrelu(conv_up2(nearest 2x)) for x4, conv_last(lrelu(conv_hr)), / img_range + mean.
// A block: y = x + proj(win_attn(qkv(LN1(x))));  x' = y + fc2(gelu(fc1(LN2(y)))), shift 4 for an odd block index.
// Weights are addressed by the reference's state-dict names.
//
// Everything this graph has in common with HAT's - the memory plan, the weight records, the head and the close of the run, the
// attention and MLP halves of a block - is WinTrunk (model_upscaler.h).  What is SwinIR's own and lives here: the 8 x 8 window attention
// on the expanded-bias derived copy of a block's table (launch_win_bias, then k_win_attn with shift 4 on the odd blocks of an image
// larger than one window), the 1conv / 3conv residual connection and the nearest+conv upsampler tail.
// Split-K factors are planned per sample (BatchInvariantScope around the run): a sample's result does not depend on its batch.
#include "model_upscaler.h"

namespace {
struct SResi { UpConv c0, c2; UpLin c1; };                                                    // 1conv: c0 alone
}  // namespace

struct gyre_swinir : WinTrunk {
    gyre_swinir_cfg cfg;
    int C4 = 0, C4p = 0;
    UpConv conv_up1, conv_up2, conv_hr;
    SResi after_body;
    std::vector<std::vector<WinAttnW>> layers;
    std::vector<SResi> resi;
    gyre_swinir() : WinTrunk("swinir") {}

    void resi_conv(const std::string& key, SResi& r) {
        if (!cfg.resi_3conv) { conv(key, C, C, Cp, Cp, r.c0); return; }
        conv(key + ".0", C4, C, C4p, Cp, r.c0);
        lin(key + ".2", C4, C4, C4p, C4p, r.c1, true);
        conv(key + ".4", C, C4, Cp, C4p, r.c2);
    }
    int build() {
        const gyre_swinir_cfg& c = cfg;
        if (c.window_size != 8) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swinir: window_size 8 is the only one built");
        TRY(configure(c, "nearest+conv"));
        C4 = C / 4; C4p = pad8(C4);
        for (int i = 0; i < c.num_layers; ++i) {
            std::vector<WinAttnW> blocks;
            for (int j = 0; j < c.depths[i]; ++j) {
                const std::string p = "layers." + std::to_string(i) + ".residual_group.blocks." + std::to_string(j);
                WinAttnW b;
                block_attn(p, 225, b);
                mlp(p, b);
                blocks.push_back(b);
            }
            layers.push_back(blocks);
            SResi r;
            resi_conv("layers." + std::to_string(i) + ".conv", r);
            resi.push_back(r);
        }
        norm("norm", &n_g, &n_b);
        resi_conv("conv_after_body", after_body);
        conv("conv_before_upsample.0", 64, C, 64, Cp, conv_bu);
        conv("conv_up1", 64, 64, 64, 64, conv_up1);
        if (c.upscale == 4) conv("conv_up2", 64, 64, 64, 64, conv_up2);
        conv("conv_hr", 64, 64, 64, 64, conv_hr);
        conv("conv_last", 3, 64, 8, 64, conv_last);
        return check_allocs();
    }

    // out = resi(x) + res  (1conv: one convolution; 3conv: 3x3 -> lrelu -> 1x1 -> lrelu -> 3x3)
    int resi_run(const SResi& r, const Tn& x, const Tn& res, Tn& out) {
        if (!cfg.resi_3conv) return conv3(x, r.c0, 0, &res, out);
        Tn t1, t2;
        TRY(ex.alloc(t1, x.B, x.H, x.W, C4p));
        TRY(conv3(x, r.c0, 0, nullptr, t1));
        TRY(act(t1, 1, 0.2f));
        TRY(ex.alloc(t2, x.B, x.H, x.W, C4p));
        TRY(linear(t1, r.c1, nullptr, t2));
        TRY(act(t2, 1, 0.2f));
        ex.free(t1);
        TRY(conv3(t2, r.c2, 0, &res, out));
        ex.free(t2);
        return 0;
    }
    // w.ao = win_attn(w.qkv) under the block's table, expanded once per weight version to the kernel's [heads][64 x 64] order
    int attention(const WinAttnW& b, int shift, Bufs& w) {
        bool fresh = false;
        float* eb = (float*)store.derived(Store::DC_WIN_BIAS, b.table, (size_t)heads * 4096 * 4, &fresh);
        if (!eb) GYRE_FAIL(GYRE_ERR_HIP, "cannot allocate the expanded relative-position bias");
        if (!fresh) TRY(launch_win_bias(ex.st, b.table, heads, eb));
        return launch_win_attn(ex.st, w.qkv.p, w.qkv.C, w.ao.p, w.ao.C, eb, w.qkv.B, w.qkv.H, w.qkv.W, heads, shift);
    }

    int run(bool dry, hipStream_t st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
        const gyre_swinir_cfg& c = cfg;
        BatchInvariantScope per_sample_plans;
        Bufs w;
        TRY(head(dry, st, img, idt, B, H, W, ws, wsb, 8, w));
        const int shift_ok = H > 8 && W > 8;
        for (int i = 0; i < c.num_layers; ++i) {
            const Tn* x = w.rin;
            for (int j = 0; j < c.depths[i]; ++j) {
                const WinAttnW& b = layers[i][j];
                const int shift = (j & 1) && shift_ok ? 4 : 0;
                TRY(attn_part(b, *x, w, *w.u, [&] { return attention(b, shift, w); }));     // y = x + proj(attn)
                TRY(mlp_part(b, *w.u, w, *w.v));                                            // x' = y + fc2(gelu(fc1(LN2(y))))
                x = w.v;
            }
            TRY(resi_run(resi[i], *x, *w.rin, *w.u));              // RSTB: conv(blocks(x)) + x
            std::swap(w.rin, w.u);
        }
        TRY(final_norm(w));
        TRY(resi_run(after_body, w.nrm, w.feat, *w.u));            // conv_after_body(norm(body)) + conv_first's output
        Tn bu, u1, u2, hr;
        TRY(before_upsample(w, bu));
        TRY(ex.alloc(u1, B, 2 * H, 2 * W, 64));
        TRY(conv3(bu, conv_up1, 1, nullptr, u1));
        TRY(act(u1, 1, 0.2f));
        ex.free(bu);
        Tn* top = &u1;
        if (c.upscale == 4) {
            TRY(ex.alloc(u2, B, 4 * H, 4 * W, 64));
            TRY(conv3(u1, conv_up2, 1, nullptr, u2));
            TRY(act(u2, 1, 0.2f));
            ex.free(u1);
            top = &u2;
        }
        TRY(ex.alloc(hr, B, top->H, top->W, 64));
        TRY(conv3(*top, conv_hr, 0, nullptr, hr));
        TRY(act(hr, 1, 0.2f));
        ex.free(*top);
        return last_and_exit(hr, out, odt);
    }
};

extern "C" {

int gyre_swinir_create(const gyre_swinir_cfg* cfg, int device, gyre_swinir** out) { return handle_create(cfg, device, out); }
void gyre_swinir_destroy(gyre_swinir* h) { delete h; }
int gyre_swinir_num_params(const gyre_swinir* h) { return handle_num_params(h); }
const char* gyre_swinir_param_key(const gyre_swinir* h, int i) { return handle_param_key(h, i); }
int gyre_swinir_set_weight(gyre_swinir* h, const char* key, const void* p, int dtype, const int64_t* shape, int ndim, void* st) {
    return handle_set_weight(h, key, p, dtype, shape, ndim, st);
}
int gyre_swinir_finalize(gyre_swinir* h, void* st) { return handle_finalize(h); }
size_t gyre_swinir_workspace_bytes(gyre_swinir* h, int B, int H, int W) { return handle_workspace_bytes(h, B, H, W); }
int gyre_swinir_forward(gyre_swinir* h, void* st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
    return handle_forward(h, "swinir", st, img, idt, B, H, W, ws, wsb, out, odt);
}

int gyre_op_win_bias(void* st, const float* table, int heads, float* out) { return launch_win_bias((hipStream_t)st, table, heads, out); }
int gyre_op_win_attn(void* st, const void* qkv, int ld_qkv, void* o, int ld_o, const float* bias, int B, int H, int W, int heads, int shift) {
    return launch_win_attn((hipStream_t)st, (const bf16_t*)qkv, ld_qkv, (bf16_t*)o, ld_o, bias, B, H, W, heads, shift);
}
int gyre_op_ln_live(void* st, const void* x, int ldx, size_t M, int C, const float* gamma, const float* beta, float eps, void* y, int ldy) {
    return launch_ln_live((hipStream_t)st, (const bf16_t*)x, ldx, M, C, gamma, beta, eps, (bf16_t*)y, ldy);
}
int gyre_op_swin_act(void* st, void* x, size_t n, int mode, float slope) { return launch_swin_act((hipStream_t)st, (bf16_t*)x, n, mode, slope); }
int gyre_op_swin_entry(void* st, const void* x, int dtype, int B, size_t HW, const float* mean3, float range, void* y) {
    return launch_swin_entry((hipStream_t)st, x, dtype, B, HW, mean3, range, (bf16_t*)y);
}
int gyre_op_swin_exit(void* st, const void* x, int ldx, int B, size_t HW, const float* mean3, float range, void* y, int dtype) {
    return launch_swin_exit((hipStream_t)st, (const bf16_t*)x, ldx, B, HW, mean3, range, y, dtype);
}

}  // extern "C"
