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
// Memory plan, as in model_swinir.hip: tokens in image order, NHWC with Cp = embed_dim rounded up to 32 channels, the CAB middle width
// C / 3 rounded up to 8; padding channels are exactly zero everywhere (zero weight rows and bias entries, zeros from the LayerNorm, the
// attention output buffer cleared once per call, the gate vector zero above C).  The qkv projections write 32-column groups per
// (q | k | v, head) (PK_MAT_HEAD30); k_hat_attn reads them through the window map and takes the position table as it is.
//
// Kernels.  Every GEMM and convolution goes through the planner (Exec::run_gemm); x + proj(attn) and both MLP residuals ride in the GEMM
// epilogues.  The CAB is two planner convolutions with launch_swin_act's GELU between them, then pool -> gate -> scale-add onto y: the
// factor conv_scale is folded into the gate vector, so y takes one fma and one more rounding.  The 1 x 1 convolutions of the channel
// attention are C x C / 30 fp32 matrices applied inside k_chan_gate.  PixelShuffle(2) is a pass of its own after each 64 -> 256
// convolution.  Split-K factors are planned per sample (gemm_set_batch_invariant(1) around the call) and the pool sums in a fixed order:
// a sample's result does not depend on its batch.
#include "model_impl.h"

namespace {
struct HConv { bf16_t* w = nullptr; float* b = nullptr; int cin = 0, cout = 0, rows = 0; };   // cin / rows: padded input channels / weight rows
struct HLin { bf16_t* w = nullptr; float* b = nullptr; int K = 0, N = 0; };                   // padded
struct HAttn { float *g1, *b1, *g2, *b2, *table; HLin qkv, proj, fc1, fc2; };                 // what a HAB and the OCAB share
struct HBlock { HAttn a; HConv cab0, cab2; float *ca_w1, *ca_b1, *ca_w2, *ca_b2; };
inline int hat_pad32(int c) { return (c + 31) / 32 * 32; }
}  // namespace

struct gyre_hat {
    gyre_hat_cfg cfg;
    Store store;
    Exec ex;
    bool finalized = false;
    int C = 0, Cp = 0, heads = 0, hid = 0, Cm = 0, Cmp = 0, Cs = 0;
    float mean[3] = {0.4488f, 0.4371f, 0.4040f};
    HConv conv_first, conv_ab, conv_bu, conv_up[2], conv_last;
    float *pe_g = nullptr, *pe_b = nullptr, *n_g = nullptr, *n_b = nullptr;
    std::vector<std::vector<HBlock>> layers;
    std::vector<HAttn> ocab;
    std::vector<HConv> resi;

    void conv(const std::string& key, int cout, int cin, int rows, int cin_pad, HConv& c) {
        c.cin = cin_pad; c.cout = cout; c.rows = rows;
        c.w = (bf16_t*)store.dmalloc((size_t)rows * 9 * cin_pad * 2, true);
        store.add(key + ".weight", {cout, cin, 3, 3}, PK_CONV3, c.w, rows, cin_pad);
        c.b = (float*)store.dmalloc((size_t)rows * 4, true);
        store.add(key + ".bias", {cout}, PK_VEC, c.b);
    }
    void lin(const std::string& key, int O, int I, int rows, int ipad, HLin& l) {
        l.K = ipad; l.N = rows;
        l.w = (bf16_t*)store.dmalloc((size_t)rows * ipad * 2, true);
        store.add(key + ".weight", {O, I}, PK_MAT, l.w, rows, ipad);
        l.b = (float*)store.dmalloc((size_t)rows * 4, true);
        store.add(key + ".bias", {O}, PK_VEC, l.b);
    }
    void norm(const std::string& key, float** g, float** b) {
        store.vec(key + ".weight", C, g);
        store.vec(key + ".bias", C, b);
    }
    void table(const std::string& key, int rows, HAttn& a) {
        a.table = (float*)store.dmalloc((size_t)rows * heads * 4, true);
        store.add(key, {rows, heads}, PK_TABLE_F32, a.table);
    }
    void qkv(const std::string& key, HAttn& a) {
        a.qkv.K = Cp; a.qkv.N = 96 * heads;
        a.qkv.w = (bf16_t*)store.dmalloc((size_t)a.qkv.N * Cp * 2, true);
        store.add(key + ".weight", {3 * C, C}, PK_MAT_HEAD30, a.qkv.w, a.qkv.N, Cp);
        a.qkv.b = (float*)store.dmalloc((size_t)a.qkv.N * 4, true);
        store.add(key + ".bias", {3 * C}, PK_VEC_HEAD30, a.qkv.b);
    }
    // a 1 x 1 convolution of the channel attention, kept in fp32 [O][I] for k_chan_gate
    void gate_mat(const std::string& key, int O, int I, float** w, float** b) {
        *w = (float*)store.dmalloc((size_t)O * I * 4, true);
        store.add(key + ".weight", {O, I, 1, 1}, PK_TABLE_F32, *w);
        store.vec(key + ".bias", O, b);
    }
    void mlp(const std::string& p, HAttn& a) {
        norm(p + ".norm2", &a.g2, &a.b2);
        lin(p + ".mlp.fc1", hid, C, hid, Cp, a.fc1);
        lin(p + ".mlp.fc2", C, hid, Cp, hid, a.fc2);
    }
    int build() {
        const gyre_hat_cfg& c = cfg;
        if (c.window_size != 16) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "hat: window_size 16 is the only one built");
        if (c.overlap_ratio != 0.5f) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "hat: overlap_ratio 0.5 is the only one built");
        if (c.compress_ratio != 3 || c.squeeze_factor != 30) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "hat: compress_ratio 3 and squeeze_factor 30 are built");
        if (c.in_chans != 3) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "hat: in_chans 3 is the only one built");
        if (c.upscale != 2 && c.upscale != 4) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "hat: pixelshuffle with upscale 2 or 4 is built");
        if (c.num_layers < 1 || c.num_layers > 16) GYRE_FAIL(GYRE_ERR_INVALID, "hat: 1 to 16 layers");
        heads = c.num_heads[0];
        for (int i = 0; i < c.num_layers; ++i) {
            if (c.num_heads[i] != heads) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "hat: the same head count in every layer is built");
            if (c.depths[i] < 1 || c.depths[i] > 64) GYRE_FAIL(GYRE_ERR_INVALID, "hat: depth out of range");
        }
        if (heads < 1 || heads > 8 || c.embed_dim != 30 * heads) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "hat: embed_dim = 30 * heads with at most 8 heads is built");
        if (c.mlp_hidden < 8 || c.mlp_hidden % 8) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "hat: the MLP width must be a multiple of 8");
        if (!(c.img_range > 0.f)) GYRE_FAIL(GYRE_ERR_INVALID, "hat: img_range must be positive");
        C = c.embed_dim; Cp = hat_pad32(C); hid = c.mlp_hidden; Cm = C / 3; Cmp = pad8(Cm); Cs = C / 30;
        ex.store = &store;
        conv("conv_first", C, 3, Cp, 8, conv_first);
        norm("patch_embed.norm", &pe_g, &pe_b);
        for (int i = 0; i < c.num_layers; ++i) {
            const std::string rg = "layers." + std::to_string(i) + ".residual_group";
            std::vector<HBlock> blocks;
            for (int j = 0; j < c.depths[i]; ++j) {
                const std::string p = rg + ".blocks." + std::to_string(j);
                HBlock b;
                norm(p + ".norm1", &b.a.g1, &b.a.b1);
                table(p + ".attn.relative_position_bias_table", 961, b.a);
                qkv(p + ".attn.qkv", b.a);
                lin(p + ".attn.proj", C, C, Cp, Cp, b.a.proj);
                conv(p + ".conv_block.cab.0", Cm, C, Cmp, Cp, b.cab0);
                conv(p + ".conv_block.cab.2", C, Cm, Cp, Cmp, b.cab2);
                gate_mat(p + ".conv_block.cab.3.attention.1", Cs, C, &b.ca_w1, &b.ca_b1);
                gate_mat(p + ".conv_block.cab.3.attention.3", C, Cs, &b.ca_w2, &b.ca_b2);
                mlp(p, b.a);
                blocks.push_back(b);
            }
            layers.push_back(blocks);
            const std::string p = rg + ".overlap_attn";
            HAttn o;
            table(p + ".relative_position_bias_table", 1521, o);
            norm(p + ".norm1", &o.g1, &o.b1);
            qkv(p + ".qkv", o);
            lin(p + ".proj", C, C, Cp, Cp, o.proj);
            mlp(p, o);
            ocab.push_back(o);
            HConv r;
            conv("layers." + std::to_string(i) + ".conv", C, C, Cp, Cp, r);
            resi.push_back(r);
        }
        norm("norm", &n_g, &n_b);
        conv("conv_after_body", C, C, Cp, Cp, conv_ab);
        conv("conv_before_upsample.0", 64, C, 64, Cp, conv_bu);
        conv("upsample.0", 256, 64, 256, 64, conv_up[0]);
        if (c.upscale == 4) conv("upsample.2", 256, 64, 256, 64, conv_up[1]);
        conv("conv_last", 3, 64, 8, 64, conv_last);
        for (void* a : store.allocs) if (!a) GYRE_FAIL(GYRE_ERR_HIP, "hipMalloc failed");
        return 0;
    }

    // a dry run plans with aligned stand-ins (arena tensors are 256-byte aligned)
    bf16_t* at(const Tn& t) const { return ex.arena.dry ? (bf16_t*)(uintptr_t)4096 : t.p; }
    // out = conv3x3(x) + bias (+ res)
    int conv3(const Tn& x, const HConv& c, const Tn* res, Tn& out) {
        if (x.C != c.cin || out.C != c.rows || out.H != x.H || out.W != x.W || out.B != x.B || (res && res->C != out.C))
            GYRE_FAIL(GYRE_ERR_INVALID, "hat: internal shape mismatch");
        GemmParams p;
        p.A = at(x); p.lda = x.C; p.mode = GEMM_CONV3;
        p.Hi = x.H; p.Wi = x.W; p.Cin = x.C; p.Ho = x.H; p.Wo = x.W; p.stride = 1; p.pad = 1; p.ups = 0;
        p.W = c.w; p.K = 9 * x.C; p.N = c.rows; p.M = x.B * x.H * x.W;
        p.bias = c.b; p.rows_per_sample = x.H * x.W;
        if (res) { p.residual = at(*res); p.ldr = res->C; }
        p.out = at(out); p.ldc = out.C; p.out_mode = OUT_BF16;
        return ex.run_gemm(p);
    }
    int linear(const Tn& x, const HLin& l, const Tn* res, Tn& out) {
        if (x.C != l.K || out.C != l.N || (res && res->C != l.N)) GYRE_FAIL(GYRE_ERR_INVALID, "hat: internal shape mismatch");
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
    struct Bufs { Tn nrm, qkv, ao, hdn, cm, c2, part, pool, gate; };
    // u = x + proj(attn(qkv(LN1(x))));  leaves LN1(x) in w.nrm
    int attn_part(const HAttn& a, int mode, int shift, const Tn& x, Bufs& w, Tn& u) {
        TRY(ln(x, a.g1, a.b1, w.nrm));
        TRY(linear(w.nrm, a.qkv, nullptr, w.qkv));
        if (!ex.dry()) TRY(launch_hat_attn(ex.st, w.qkv.p, w.qkv.C, w.ao.p, w.ao.C, a.table, mode, x.B, x.H, x.W, heads, shift));
        return linear(w.ao, a.proj, &x, u);
    }
    // v = u + fc2(gelu(fc1(LN2(u))))
    int mlp_part(const HAttn& a, Tn& u, Bufs& w, Tn& v) {
        TRY(ln(u, a.g2, a.b2, w.nrm));
        TRY(linear(w.nrm, a.fc1, nullptr, w.hdn));
        TRY(act(w.hdn, 0, 0.f));
        return linear(w.hdn, a.fc2, &u, v);
    }
    // u += conv_scale * CAB(w.nrm)
    int cab_part(const HBlock& b, Bufs& w, Tn& u) {
        TRY(conv3(w.nrm, b.cab0, nullptr, w.cm));
        TRY(act(w.cm, 0, 0.f));
        TRY(conv3(w.cm, b.cab2, nullptr, w.c2));
        if (ex.dry()) return 0;
        const size_t HW = (size_t)u.H * u.W;
        TRY(launch_chan_pool(ex.st, w.c2.p, w.c2.C, u.B, HW, C, (float*)w.part.p, (float*)w.pool.p));
        TRY(launch_chan_gate(ex.st, (const float*)w.pool.p, u.B, C, Cs, b.ca_w1, b.ca_b1, b.ca_w2, b.ca_b2, cfg.conv_scale, (float*)w.gate.p, Cp));
        return launch_scale_add(ex.st, u.p, u.C, w.c2.p, w.c2.C, (const float*)w.gate.p, Cp, u.B, HW, Cp);
    }

    int run(bool dry, hipStream_t st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
        const gyre_hat_cfg& c = cfg;
        if (B < 1 || H < 16 || W < 16 || H % 16 || W % 16) GYRE_FAIL(GYRE_ERR_INVALID, "hat: H and W must be positive multiples of the window size 16");
        ex.arena.reset((char*)ws, wsb, dry); ex.st = st; ex.batch = B; ex.cs_unit = 0;
        Tn x0, feat, a, t1, t2;
        Bufs w;
        TRY(ex.alloc(x0, B, H, W, 8));
        if (!dry) TRY(launch_swin_entry(st, img, idt, B, (size_t)H * W, mean, c.img_range, x0.p));
        TRY(ex.alloc(feat, B, H, W, Cp));
        TRY(conv3(x0, conv_first, nullptr, feat));
        ex.free(x0);
        TRY(ex.alloc(a, B, H, W, Cp));
        TRY(ex.alloc(t1, B, H, W, Cp));
        TRY(ex.alloc(t2, B, H, W, Cp));
        TRY(ex.alloc(w.nrm, B, H, W, Cp));
        TRY(ex.alloc(w.qkv, B, H, W, 96 * heads));
        TRY(ex.alloc(w.ao, B, H, W, Cp));
        TRY(ex.alloc(w.hdn, B, H, W, hid));
        TRY(ex.alloc(w.cm, B, H, W, Cmp));
        TRY(ex.alloc(w.c2, B, H, W, Cp));
        TRY(ex.alloc(w.part, 1, 1, 1, (int)chan_pool_partial_floats(B, (size_t)H * W, C), 4));
        TRY(ex.alloc(w.pool, B, 1, 1, C, 4));
        TRY(ex.alloc(w.gate, B, 1, 1, Cp, 4));
        if (!dry) GYRE_HIP_CHECK(hipMemsetAsync(w.ao.p, 0, w.ao.bytes, st));     // the padding columns [C, Cp) stay zero: the kernel never writes them
        TRY(ln(feat, pe_g, pe_b, a));
        Tn *rin = &a, *u = &t1, *v = &t2;            // RHAG input, and the two tensors its blocks alternate between
        for (int i = 0; i < c.num_layers; ++i) {
            const Tn* x = rin;
            for (int j = 0; j < c.depths[i]; ++j) {
                const HBlock& b = layers[i][j];
                TRY(attn_part(b.a, HAT_ATTN_SA, (j & 1) ? 8 : 0, *x, w, *u));    // y = x + proj(attn)
                TRY(cab_part(b, w, *u));                                         // y += conv_scale * CAB(LN1(x))
                TRY(mlp_part(b.a, *u, w, *v));
                x = v;
            }
            TRY(attn_part(ocab[i], HAT_ATTN_OCA, 0, *x, w, *u));
            TRY(mlp_part(ocab[i], *u, w, *v));
            TRY(conv3(*v, resi[i], rin, *u));                                    // RHAG: conv(OCAB(HABs(x))) + x
            std::swap(rin, u);
        }
        TRY(ln(*rin, n_g, n_b, w.nrm));
        ex.free(w.qkv); ex.free(w.ao); ex.free(w.hdn); ex.free(w.cm); ex.free(w.c2); ex.free(w.part); ex.free(w.pool); ex.free(w.gate);
        TRY(conv3(w.nrm, conv_ab, &feat, *u));                                   // conv_after_body(norm(body)) + conv_first's output
        ex.free(w.nrm); ex.free(feat); ex.free(*rin); ex.free(*v);
        Tn cur, wide, last;
        TRY(ex.alloc(cur, B, H, W, 64));
        TRY(conv3(*u, conv_bu, nullptr, cur));
        TRY(act(cur, 1, 0.01f));                                                 // nn.LeakyReLU(inplace=True): the default slope
        ex.free(*u);
        for (int k = 0; k < (c.upscale == 4 ? 2 : 1); ++k) {
            Tn next;
            TRY(ex.alloc(wide, B, cur.H, cur.W, 256));
            TRY(conv3(cur, conv_up[k], nullptr, wide));
            TRY(ex.alloc(next, B, 2 * cur.H, 2 * cur.W, 64));
            if (!dry) TRY(launch_pixel_shuffle2(st, wide.p, 256, B, cur.H, cur.W, 64, next.p, 64));
            ex.free(wide); ex.free(cur);
            cur = next;
        }
        TRY(ex.alloc(last, B, cur.H, cur.W, 8));
        TRY(conv3(cur, conv_last, nullptr, last));
        ex.free(cur);
        if (!dry) {
            if (!out) GYRE_FAIL(GYRE_ERR_INVALID, "hat: null output buffer");
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

int gyre_hat_create(const gyre_hat_cfg* cfg, int device, gyre_hat** out) { return handle_create(cfg, device, out); }
void gyre_hat_destroy(gyre_hat* h) { delete h; }
int gyre_hat_num_params(const gyre_hat* h) { return handle_num_params(h); }
const char* gyre_hat_param_key(const gyre_hat* h, int i) { return handle_param_key(h, i); }
int gyre_hat_set_weight(gyre_hat* h, const char* key, const void* p, int dtype, const int64_t* shape, int ndim, void* st) {
    if (!h || !key || !p || !shape) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    h->finalized = false;
    return h->store.set_weight(key, p, dtype, shape, ndim, (hipStream_t)st);
}
int gyre_hat_finalize(gyre_hat* h, void* st) { return handle_finalize(h); }
size_t gyre_hat_workspace_bytes(gyre_hat* h, int B, int H, int W) {
    if (!h) return 0;
    return h->run_invariant(true, nullptr, nullptr, 0, B, H, W, nullptr, 0, nullptr, 0) ? 0 : h->ex.arena.peak;
}
int gyre_hat_forward(gyre_hat* h, void* st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
    if (!h || !img || !ws || !out) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    if (!h->finalized) GYRE_FAIL(GYRE_ERR_INCOMPLETE, "gyre_hat_finalize has not succeeded");
    if (idt < 0 || idt > 2 || odt < 0 || odt > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    gyre_launch_counter() = 0;
    return h->run_invariant(false, (hipStream_t)st, img, idt, B, H, W, ws, wsb, out, odt);
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
