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
// Memory plan.  Tokens stay in image order, NHWC with Cp = embed_dim rounded up to 32 channels (180 -> 192, 240 -> 256); the padding
// channels are exactly zero everywhere: zero weight rows and bias entries in every producer, zeros written by the LayerNorm, and the
// attention output buffer - whose padding columns the kernel never writes - is cleared once per call.  The qkv projection writes
// 32-column groups per (q | k | v, head) (PK_MAT_HEAD30); k_win_attn reads them through the window / shift map, so no rolled or
// partitioned copy exists.  Three Cp-channel tensors rotate through an RSTB: its input (kept for the closing residual) and the two the
// blocks alternate between.
//
// Kernels.  Every GEMM and convolution goes through the planner (Exec::run_gemm); residual additions ride in the GEMM epilogues.  The
// LayerNorms are the stand-alone launch_ln_live: the planner's folded form takes its statistics over the whole K = Cp row, which is not
// the live-channel mean, so the fold does not apply to a padded width.  GELU and the leaky ReLUs are in-place passes (launch_swin_act).
// Split-K factors are planned per sample (gemm_set_batch_invariant(1) around the call): a sample's result does not depend on its batch.
#include "model_impl.h"

namespace {
struct SConv { bf16_t* w = nullptr; float* b = nullptr; int cin = 0, cout = 0, rows = 0; };   // cin / rows: padded input channels / weight rows
struct SLin { bf16_t* w = nullptr; float* b = nullptr; int K = 0, N = 0; };                   // padded
struct SResi { SConv c0, c2; SLin c1; };                                                      // 1conv: c0 alone
struct SBlock { float *g1, *b1, *g2, *b2, *table; SLin qkv, proj, fc1, fc2; };
inline int pad32(int c) { return (c + 31) / 32 * 32; }
}  // namespace

struct gyre_swinir {
    gyre_swinir_cfg cfg;
    Store store;
    Exec ex;
    bool finalized = false;
    int C = 0, Cp = 0, heads = 0, hid = 0, C4 = 0, C4p = 0;
    float mean[3] = {0.4488f, 0.4371f, 0.4040f};
    SConv conv_first, conv_bu, conv_up1, conv_up2, conv_hr, conv_last;
    SResi after_body;
    float *pe_g = nullptr, *pe_b = nullptr, *n_g = nullptr, *n_b = nullptr;
    std::vector<std::vector<SBlock>> layers;
    std::vector<SResi> resi;

    void conv(const std::string& key, int cout, int cin, int rows, int cin_pad, SConv& c) {
        c.cin = cin_pad; c.cout = cout; c.rows = rows;
        c.w = (bf16_t*)store.dmalloc((size_t)rows * 9 * cin_pad * 2, true);
        store.add(key + ".weight", {cout, cin, 3, 3}, PK_CONV3, c.w, rows, cin_pad);
        c.b = (float*)store.dmalloc((size_t)rows * 4, true);
        store.add(key + ".bias", {cout}, PK_VEC, c.b);
    }
    void lin(const std::string& key, int O, int I, int rows, int ipad, bool conv1x1, SLin& l) {
        l.K = ipad; l.N = rows;
        l.w = (bf16_t*)store.dmalloc((size_t)rows * ipad * 2, true);
        store.add(key + ".weight", conv1x1 ? std::vector<int64_t>{O, I, 1, 1} : std::vector<int64_t>{O, I}, PK_MAT, l.w, rows, ipad);
        l.b = (float*)store.dmalloc((size_t)rows * 4, true);
        store.add(key + ".bias", {O}, PK_VEC, l.b);
    }
    void resi_conv(const std::string& key, SResi& r) {
        if (!cfg.resi_3conv) { conv(key, C, C, Cp, Cp, r.c0); return; }
        conv(key + ".0", C4, C, C4p, Cp, r.c0);
        lin(key + ".2", C4, C4, C4p, C4p, true, r.c1);
        conv(key + ".4", C, C4, Cp, C4p, r.c2);
    }
    int build() {
        const gyre_swinir_cfg& c = cfg;
        if (c.window_size != 8) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swinir: window_size 8 is the only one built");
        if (c.in_chans != 3) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swinir: in_chans 3 is the only one built");
        if (c.upscale != 2 && c.upscale != 4) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swinir: nearest+conv with upscale 2 or 4 is built");
        if (c.num_layers < 1 || c.num_layers > 16) GYRE_FAIL(GYRE_ERR_INVALID, "swinir: 1 to 16 layers");
        heads = c.num_heads[0];
        for (int i = 0; i < c.num_layers; ++i) {
            if (c.num_heads[i] != heads) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swinir: the same head count in every layer is built");
            if (c.depths[i] < 1 || c.depths[i] > 64) GYRE_FAIL(GYRE_ERR_INVALID, "swinir: depth out of range");
        }
        if (heads < 1 || heads > 8 || c.embed_dim != 30 * heads) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swinir: embed_dim = 30 * heads with at most 8 heads is built");
        if (c.mlp_hidden < 8 || c.mlp_hidden % 8) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "swinir: the MLP width must be a multiple of 8");
        if (!(c.img_range > 0.f)) GYRE_FAIL(GYRE_ERR_INVALID, "swinir: img_range must be positive");
        C = c.embed_dim; Cp = pad32(C); hid = c.mlp_hidden; C4 = C / 4; C4p = pad8(C4);
        ex.store = &store;
        conv("conv_first", C, 3, Cp, 8, conv_first);
        store.vec("patch_embed.norm.weight", C, &pe_g);
        store.vec("patch_embed.norm.bias", C, &pe_b);
        for (int i = 0; i < c.num_layers; ++i) {
            std::vector<SBlock> blocks;
            for (int j = 0; j < c.depths[i]; ++j) {
                const std::string p = "layers." + std::to_string(i) + ".residual_group.blocks." + std::to_string(j);
                SBlock b;
                store.vec(p + ".norm1.weight", C, &b.g1);
                store.vec(p + ".norm1.bias", C, &b.b1);
                b.table = (float*)store.dmalloc((size_t)225 * heads * 4, true);
                store.add(p + ".attn.relative_position_bias_table", {225, heads}, PK_TABLE_F32, b.table);
                b.qkv.K = Cp; b.qkv.N = 96 * heads;
                b.qkv.w = (bf16_t*)store.dmalloc((size_t)b.qkv.N * Cp * 2, true);
                store.add(p + ".attn.qkv.weight", {3 * C, C}, PK_MAT_HEAD30, b.qkv.w, b.qkv.N, Cp);
                b.qkv.b = (float*)store.dmalloc((size_t)b.qkv.N * 4, true);
                store.add(p + ".attn.qkv.bias", {3 * C}, PK_VEC_HEAD30, b.qkv.b);
                lin(p + ".attn.proj", C, C, Cp, Cp, false, b.proj);
                store.vec(p + ".norm2.weight", C, &b.g2);
                store.vec(p + ".norm2.bias", C, &b.b2);
                lin(p + ".mlp.fc1", hid, C, hid, Cp, false, b.fc1);
                lin(p + ".mlp.fc2", C, hid, Cp, hid, false, b.fc2);
                blocks.push_back(b);
            }
            layers.push_back(blocks);
            SResi r;
            resi_conv("layers." + std::to_string(i) + ".conv", r);
            resi.push_back(r);
        }
        store.vec("norm.weight", C, &n_g);
        store.vec("norm.bias", C, &n_b);
        resi_conv("conv_after_body", after_body);
        conv("conv_before_upsample.0", 64, C, 64, Cp, conv_bu);
        conv("conv_up1", 64, 64, 64, 64, conv_up1);
        if (c.upscale == 4) conv("conv_up2", 64, 64, 64, 64, conv_up2);
        conv("conv_hr", 64, 64, 64, 64, conv_hr);
        conv("conv_last", 3, 64, 8, 64, conv_last);
        for (void* a : store.allocs) if (!a) GYRE_FAIL(GYRE_ERR_HIP, "hipMalloc failed");
        return 0;
    }

    // a dry run plans with aligned stand-ins (arena tensors are 256-byte aligned)
    bf16_t* at(const Tn& t) const { return ex.arena.dry ? (bf16_t*)(uintptr_t)4096 : t.p; }
    // out = conv3x3(x) + bias (+ res); ups: nearest 2x inside the gather
    int conv3(const Tn& x, const SConv& c, int ups, const Tn* res, Tn& out) {
        const int Ho = ups ? 2 * x.H : x.H, Wo = ups ? 2 * x.W : x.W;
        if (x.C != c.cin || out.C != c.rows || out.H != Ho || out.W != Wo || out.B != x.B || (res && res->C != out.C))
            GYRE_FAIL(GYRE_ERR_INVALID, "swinir: internal shape mismatch");
        GemmParams p;
        p.A = at(x); p.lda = x.C; p.mode = GEMM_CONV3;
        p.Hi = x.H; p.Wi = x.W; p.Cin = x.C; p.Ho = Ho; p.Wo = Wo; p.stride = 1; p.pad = 1; p.ups = ups;
        p.Hup = ups ? Ho : 0; p.Wup = ups ? Wo : 0;
        p.W = c.w; p.K = 9 * x.C; p.N = c.rows; p.M = x.B * Ho * Wo;
        p.bias = c.b; p.rows_per_sample = Ho * Wo;
        if (res) { p.residual = at(*res); p.ldr = res->C; }
        p.out = at(out); p.ldc = out.C; p.out_mode = OUT_BF16;
        return ex.run_gemm(p);
    }
    int linear(const Tn& x, const SLin& l, const Tn* res, Tn& out) {
        if (x.C != l.K || out.C != l.N || (res && res->C != l.N)) GYRE_FAIL(GYRE_ERR_INVALID, "swinir: internal shape mismatch");
        return ex.linear(at(x), x.C, nullptr, 0, 0, x.rows(), l.K, l.w, l.N, l.b, res ? at(*res) : nullptr, res ? res->C : 0, 0, at(out), out.C);
    }
    int act(Tn& t, int mode, float slope) {
        if (ex.dry()) return 0;
        return launch_swin_act(ex.st, t.p, (size_t)t.rows() * t.C, mode, slope);
    }
    int ln(const Tn& x, const float* g, const float* b, Tn& y) {
        if (ex.dry()) return 0;
        return launch_ln_live(ex.st, x.p, x.C, (size_t)x.rows(), C, g, b, 1e-5f, y.p, y.C);
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

    int run(bool dry, hipStream_t st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
        const gyre_swinir_cfg& c = cfg;
        if (B < 1 || H < 8 || W < 8 || H % 8 || W % 8) GYRE_FAIL(GYRE_ERR_INVALID, "swinir: H and W must be positive multiples of the window size 8");
        ex.arena.reset((char*)ws, wsb, dry); ex.st = st; ex.batch = B; ex.cs_unit = 0;
        Tn x0, feat, a, t1, t2, nrm, qkv, ao, hdn;
        TRY(ex.alloc(x0, B, H, W, 8));
        if (!dry) TRY(launch_swin_entry(st, img, idt, B, (size_t)H * W, mean, c.img_range, x0.p));
        TRY(ex.alloc(feat, B, H, W, Cp));
        TRY(conv3(x0, conv_first, 0, nullptr, feat));
        ex.free(x0);
        TRY(ex.alloc(a, B, H, W, Cp));
        TRY(ex.alloc(t1, B, H, W, Cp));
        TRY(ex.alloc(t2, B, H, W, Cp));
        TRY(ex.alloc(nrm, B, H, W, Cp));
        TRY(ex.alloc(qkv, B, H, W, 96 * heads));
        TRY(ex.alloc(ao, B, H, W, Cp));
        TRY(ex.alloc(hdn, B, H, W, hid));
        if (!dry) GYRE_HIP_CHECK(hipMemsetAsync(ao.p, 0, ao.bytes, st));     // the padding columns [C, Cp) stay zero: the kernel never writes them
        TRY(ln(feat, pe_g, pe_b, a));
        Tn *rin = &a, *u = &t1, *v = &t2;            // RSTB input, and the two tensors its blocks alternate between
        const int shift_ok = H > 8 && W > 8;
        for (int i = 0; i < c.num_layers; ++i) {
            const Tn* x = rin;
            for (int j = 0; j < c.depths[i]; ++j) {
                const SBlock& b = layers[i][j];
                TRY(ln(*x, b.g1, b.b1, nrm));
                TRY(linear(nrm, b.qkv, nullptr, qkv));
                if (!dry) {
                    bool fresh = false;
                    float* eb = (float*)store.derived(Store::DC_WIN_BIAS, b.table, (size_t)heads * 4096 * 4, &fresh);
                    if (!eb) GYRE_FAIL(GYRE_ERR_HIP, "cannot allocate the expanded relative-position bias");
                    if (!fresh) TRY(launch_win_bias(st, b.table, heads, eb));
                    TRY(launch_win_attn(st, qkv.p, qkv.C, ao.p, ao.C, eb, B, H, W, heads, (j & 1) && shift_ok ? 4 : 0));
                }
                TRY(linear(ao, b.proj, x, *u));                  // y = x + proj(attn)
                TRY(ln(*u, b.g2, b.b2, nrm));
                TRY(linear(nrm, b.fc1, nullptr, hdn));
                TRY(act(hdn, 0, 0.f));
                TRY(linear(hdn, b.fc2, u, *v));                  // x' = y + fc2(gelu(fc1(LN2(y))))
                x = v;
            }
            TRY(resi_run(resi[i], *x, *rin, *u));                // RSTB: conv(blocks(x)) + x
            std::swap(rin, u);
        }
        TRY(ln(*rin, n_g, n_b, nrm));
        ex.free(qkv); ex.free(ao); ex.free(hdn);
        TRY(resi_run(after_body, nrm, feat, *u));                // conv_after_body(norm(body)) + conv_first's output
        ex.free(nrm); ex.free(feat); ex.free(*rin); ex.free(*v);
        Tn bu, u1, u2, hr, last;
        TRY(ex.alloc(bu, B, H, W, 64));
        TRY(conv3(*u, conv_bu, 0, nullptr, bu));
        TRY(act(bu, 1, 0.01f));                                  // nn.LeakyReLU(inplace=True): the default slope
        ex.free(*u);
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
        TRY(ex.alloc(last, B, hr.H, hr.W, 8));
        TRY(conv3(hr, conv_last, 0, nullptr, last));
        ex.free(hr);
        if (!dry) {
            if (!out) GYRE_FAIL(GYRE_ERR_INVALID, "swinir: null output buffer");
            TRY(launch_swin_exit(st, last.p, last.C, B, (size_t)last.H * last.W, mean, c.img_range, out, odt));
        }
        ex.free(last);
        return 0;
    }
    // the planner sees every launch as if its sample ran alone: no batch-dependent split-K factor
    int run_invariant(bool dry, hipStream_t st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
        const int prev = gemm_set_batch_invariant(1);
        const int rc = run(dry, st, img, idt, B, H, W, ws, wsb, out, odt);
        gemm_set_batch_invariant(prev);
        return rc;
    }
};

extern "C" {

int gyre_swinir_create(const gyre_swinir_cfg* cfg, int device, gyre_swinir** out) { return handle_create(cfg, device, out); }
void gyre_swinir_destroy(gyre_swinir* h) { delete h; }
int gyre_swinir_num_params(const gyre_swinir* h) { return handle_num_params(h); }
const char* gyre_swinir_param_key(const gyre_swinir* h, int i) { return handle_param_key(h, i); }
int gyre_swinir_set_weight(gyre_swinir* h, const char* key, const void* p, int dtype, const int64_t* shape, int ndim, void* st) {
    if (!h || !key || !p || !shape) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    h->finalized = false;
    return h->store.set_weight(key, p, dtype, shape, ndim, (hipStream_t)st);
}
int gyre_swinir_finalize(gyre_swinir* h, void* st) { return handle_finalize(h); }
size_t gyre_swinir_workspace_bytes(gyre_swinir* h, int B, int H, int W) {
    if (!h) return 0;
    return h->run_invariant(true, nullptr, nullptr, 0, B, H, W, nullptr, 0, nullptr, 0) ? 0 : h->ex.arena.peak;
}
int gyre_swinir_forward(gyre_swinir* h, void* st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
    if (!h || !img || !ws || !out) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    if (!h->finalized) GYRE_FAIL(GYRE_ERR_INCOMPLETE, "gyre_swinir_finalize has not succeeded");
    if (idt < 0 || idt > 2 || odt < 0 || odt > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    gyre_launch_counter() = 0;
    return h->run_invariant(false, (hipStream_t)st, img, idt, B, H, W, ws, wsb, out, odt);
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
