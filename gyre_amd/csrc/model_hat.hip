// HAT upscaler graph and its C ABI (include/gyre_hip.h).
//
// Topology restates the reference's vendored model (gyre/pipeline/upscalers/models/hat_arch.py, HAT.forward with upsampler
// "pixelshuffle", lines 976-989; HAB.forward 271-314, OCAB.forward 397-443, RHAG.forward 623-624):
//   (x - mean) * img_range, conv_first, patch_embed.norm, per RHAG: HABs, OCAB, then conv + the RHAG input, norm,
//   conv_after_body + conv_first's output, lrelu_0.01(conv_before_upsample.0), per factor of 2: conv 64 -> 256 and PixelShuffle(2),
//   conv_last, / img_range + mean.  There is no padding: H and W are multiples of 16, as the reference requires.
// HAB:  n = LN1(x);  y = x + proj(win_attn16(qkv(n))) + conv_scale * CAB(n);  x' = y + fc2(gelu(fc1(LN2(y)))); shift 8 for an odd
//       block index whatever the image size (the reference's blocks are built for img_size 64, not for the image).
// CAB:  c = conv3x3(gelu(conv3x3(n)));  c * sigmoid(W2 relu(W1 mean_HW(c) + b1) + b2)  - the mean over the whole image.
// OCAB: y = x + proj(overlap_attn(qkv(LN1(x))));  x' = y + fc2(gelu(fc1(LN2(y)))).
// Weights are addressed by the reference's state-dict names.
//
// Everything this graph has in common with SwinIR's - the memory plan, the weight records, the head and the close of the run, the
// attention and MLP halves of a block - is WinTrunk (model_upscaler.h).  What is HAT's own and lives here: the 16 x 16 and the
// overlapping window attention (k_hat_attn takes the position table as it is and always shifts the odd blocks), the CAB, the OCAB step
// that closes every group and the pixel-shuffle tail.  The CAB middle width is C / 3 rounded up to 8; the gate vector is zero above C.
//
// The CAB is two planner convolutions with launch_swin_act's GELU between them, then pool -> gate -> scale-add onto y: the factor
// conv_scale is folded into the gate vector, so y takes one fma and one more rounding.  The 1 x 1 convolutions of the channel attention
// are C x C / 30 fp32 matrices applied inside k_chan_gate.  PixelShuffle(2) is a pass of its own after each 64 -> 256 convolution.
// Split-K factors are planned per sample (BatchInvariantScope around the run) and the pool sums in a fixed order: a sample's result does
// not depend on its batch.
#include "model_upscaler.h"

namespace {
struct HBlock { WinAttnW a; UpConv cab0, cab2; float *ca_w1, *ca_b1, *ca_w2, *ca_b2; };
}  // namespace

struct gyre_hat : WinTrunk {
    gyre_hat_cfg cfg;
    int Cm = 0, Cmp = 0, Cs = 0;
    UpConv conv_ab, conv_up[2];
    std::vector<std::vector<HBlock>> layers;
    std::vector<WinAttnW> ocab;
    std::vector<UpConv> resi;
    gyre_hat() : WinTrunk("hat") {}

    // a 1 x 1 convolution of the channel attention, kept in fp32 [O][I] for k_chan_gate
    void gate_mat(const std::string& key, int O, int I, float** w, float** b) {
        *w = (float*)store.dmalloc((size_t)O * I * 4, true);
        store.add(key + ".weight", {O, I, 1, 1}, PK_TABLE_F32, *w);
        store.vec(key + ".bias", O, b);
    }
    int build() {
        const gyre_hat_cfg& c = cfg;
        if (c.window_size != 16) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "hat: window_size 16 is the only one built");
        if (c.overlap_ratio != 0.5f) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "hat: overlap_ratio 0.5 is the only one built");
        if (c.compress_ratio != 3 || c.squeeze_factor != 30) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "hat: compress_ratio 3 and squeeze_factor 30 are built");
        TRY(configure(c, "pixelshuffle"));
        Cm = C / 3; Cmp = pad8(Cm); Cs = C / 30;
        for (int i = 0; i < c.num_layers; ++i) {
            const std::string rg = "layers." + std::to_string(i) + ".residual_group";
            std::vector<HBlock> blocks;
            for (int j = 0; j < c.depths[i]; ++j) {
                const std::string p = rg + ".blocks." + std::to_string(j);
                HBlock b;
                block_attn(p, 961, b.a);
                conv(p + ".conv_block.cab.0", Cm, C, Cmp, Cp, b.cab0);
                conv(p + ".conv_block.cab.2", C, Cm, Cp, Cmp, b.cab2);
                gate_mat(p + ".conv_block.cab.3.attention.1", Cs, C, &b.ca_w1, &b.ca_b1);
                gate_mat(p + ".conv_block.cab.3.attention.3", C, Cs, &b.ca_w2, &b.ca_b2);
                mlp(p, b.a);
                blocks.push_back(b);
            }
            layers.push_back(blocks);
            const std::string p = rg + ".overlap_attn";
            WinAttnW o;
            table(p + ".relative_position_bias_table", 1521, o);
            norm(p + ".norm1", &o.g1, &o.b1);
            qkv_proj(p, o);
            mlp(p, o);
            ocab.push_back(o);
            UpConv r;
            conv("layers." + std::to_string(i) + ".conv", C, C, Cp, Cp, r);
            resi.push_back(r);
        }
        norm("norm", &n_g, &n_b);
        conv("conv_after_body", C, C, Cp, Cp, conv_ab);
        conv("conv_before_upsample.0", 64, C, 64, Cp, conv_bu);
        conv("upsample.0", 256, 64, 256, 64, conv_up[0]);
        if (c.upscale == 4) conv("upsample.2", 256, 64, 256, 64, conv_up[1]);
        conv("conv_last", 3, 64, 8, 64, conv_last);
        return check_allocs();
    }

    struct CabBufs { Tn cm, c2, part, pool, gate; };
    // u = x + proj(attn(qkv(LN1(x)))) with k_hat_attn in the given mode
    int attn_part(const WinAttnW& a, int mode, int shift, const Tn& x, Bufs& w, Tn& u) {
        return WinTrunk::attn_part(a, x, w, u, [&] {
            return launch_hat_attn(ex.st, w.qkv.p, w.qkv.C, w.ao.p, w.ao.C, a.table, mode, x.B, x.H, x.W, heads, shift);
        });
    }
    // u += conv_scale * CAB(w.nrm)
    int cab_part(const HBlock& b, Bufs& w, CabBufs& k, Tn& u) {
        TRY(conv3(w.nrm, b.cab0, 0, nullptr, k.cm));
        TRY(act(k.cm, 0, 0.f));
        TRY(conv3(k.cm, b.cab2, 0, nullptr, k.c2));
        if (ex.dry()) return 0;
        const size_t HW = (size_t)u.H * u.W;
        TRY(launch_chan_pool(ex.st, k.c2.p, k.c2.C, u.B, HW, C, (float*)k.part.p, (float*)k.pool.p));
        TRY(launch_chan_gate(ex.st, (const float*)k.pool.p, u.B, C, Cs, b.ca_w1, b.ca_b1, b.ca_w2, b.ca_b2, cfg.conv_scale, (float*)k.gate.p, Cp));
        return launch_scale_add(ex.st, u.p, u.C, k.c2.p, k.c2.C, (const float*)k.gate.p, Cp, u.B, HW, Cp);
    }

    int run(bool dry, hipStream_t st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
        const gyre_hat_cfg& c = cfg;
        BatchInvariantScope per_sample_plans;
        Bufs w;
        CabBufs k;
        TRY(head(dry, st, img, idt, B, H, W, ws, wsb, 16, w));
        TRY(ex.alloc(k.cm, B, H, W, Cmp));
        TRY(ex.alloc(k.c2, B, H, W, Cp));
        TRY(ex.alloc(k.part, 1, 1, 1, (int)chan_pool_partial_floats(B, (size_t)H * W, C), 4));
        TRY(ex.alloc(k.pool, B, 1, 1, C, 4));
        TRY(ex.alloc(k.gate, B, 1, 1, Cp, 4));
        for (int i = 0; i < c.num_layers; ++i) {
            const Tn* x = w.rin;
            for (int j = 0; j < c.depths[i]; ++j) {
                const HBlock& b = layers[i][j];
                TRY(attn_part(b.a, HAT_ATTN_SA, (j & 1) ? 8 : 0, *x, w, *w.u));  // y = x + proj(attn)
                TRY(cab_part(b, w, k, *w.u));                                    // y += conv_scale * CAB(LN1(x))
                TRY(mlp_part(b.a, *w.u, w, *w.v));
                x = w.v;
            }
            TRY(attn_part(ocab[i], HAT_ATTN_OCA, 0, *x, w, *w.u));
            TRY(mlp_part(ocab[i], *w.u, w, *w.v));
            TRY(conv3(*w.v, resi[i], 0, w.rin, *w.u));                           // RHAG: conv(OCAB(HABs(x))) + x
            std::swap(w.rin, w.u);
        }
        TRY(final_norm(w));
        ex.free(k.cm); ex.free(k.c2); ex.free(k.part); ex.free(k.pool); ex.free(k.gate);
        TRY(conv3(w.nrm, conv_ab, 0, &w.feat, *w.u));                            // conv_after_body(norm(body)) + conv_first's output
        Tn cur, wide;
        TRY(before_upsample(w, cur));
        for (int n = 0; n < (c.upscale == 4 ? 2 : 1); ++n) {
            Tn next;
            TRY(ex.alloc(wide, B, cur.H, cur.W, 256));
            TRY(conv3(cur, conv_up[n], 0, nullptr, wide));
            TRY(ex.alloc(next, B, 2 * cur.H, 2 * cur.W, 64));
            if (!dry) TRY(launch_pixel_shuffle2(st, wide.p, 256, B, cur.H, cur.W, 64, next.p, 64));
            ex.free(wide); ex.free(cur);
            cur = next;
        }
        return last_and_exit(cur, out, odt);
    }
};

extern "C" {

int gyre_hat_create(const gyre_hat_cfg* cfg, int device, gyre_hat** out) { return handle_create(cfg, device, out); }
void gyre_hat_destroy(gyre_hat* h) { delete h; }
int gyre_hat_num_params(const gyre_hat* h) { return handle_num_params(h); }
const char* gyre_hat_param_key(const gyre_hat* h, int i) { return handle_param_key(h, i); }
int gyre_hat_set_weight(gyre_hat* h, const char* key, const void* p, int dtype, const int64_t* shape, int ndim, void* st) {
    return handle_set_weight(h, key, p, dtype, shape, ndim, st);
}
int gyre_hat_finalize(gyre_hat* h, void* st) { return handle_finalize(h); }
size_t gyre_hat_workspace_bytes(gyre_hat* h, int B, int H, int W) { return handle_workspace_bytes(h, B, H, W); }
int gyre_hat_forward(gyre_hat* h, void* st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
    return handle_forward(h, "hat", st, img, idt, B, H, W, ws, wsb, out, odt);
}

int gyre_op_hat_attn(void* st, const void* qkv, int ld_qkv, void* o, int ld_o, const float* table, int mode, int B, int H, int W, int heads,
                     int shift) {
    return launch_hat_attn((hipStream_t)st, (const bf16_t*)qkv, ld_qkv, (bf16_t*)o, ld_o, table, mode, B, H, W, heads, shift);
}
size_t gyre_op_chan_pool_workspace(int B, size_t HW, int C) { return chan_pool_partial_floats(B, HW, C) * sizeof(float); }
int gyre_op_chan_pool(void* st, const void* x, int ld, int B, size_t HW, int C, float* partial, float* pool) {
    return launch_chan_pool((hipStream_t)st, (const bf16_t*)x, ld, B, HW, C, partial, pool);
}
int gyre_op_chan_gate(void* st, const float* pool, int B, int C, int Cs, const float* w1, const float* b1, const float* w2, const float* b2,
                      float scale, float* s, int ld_s) {
    return launch_chan_gate((hipStream_t)st, pool, B, C, Cs, w1, b1, w2, b2, scale, s, ld_s);
}
int gyre_op_scale_add(void* st, void* y, int ldy, const void* c2, int ldc, const float* s, int ld_s, int B, size_t HW, int Cn) {
    return launch_scale_add((hipStream_t)st, (bf16_t*)y, ldy, (const bf16_t*)c2, ldc, s, ld_s, B, HW, Cn);
}
int gyre_op_pixel_shuffle2(void* st, const void* x, int ld_x, int B, int H, int W, int Co, void* out, int ld_out) {
    return launch_pixel_shuffle2((hipStream_t)st, (const bf16_t*)x, ld_x, B, H, W, Co, (bf16_t*)out, ld_out);
}

}  // extern "C"
