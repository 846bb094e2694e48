// The line-art hinter graph and its C ABI (include/gyre_hip.h): the reference's DrawingGenerator (gyre/pipeline/hinters/models/
// informative_drawings.py, the informative-drawings generator), which it serves three times (config/models/hinters.yaml:
// hinters-lineart-anime / -contour / -opensketch) as DrawingGenerator(3, 1, n_residual_blocks=3) behind InformativeDrawingPipeline.
//
// Topology, with IN = the affine-free InstanceNorm2d and every tensor NHWC in the storage type:
//   model0   reflect 3, conv 7x7 3 -> 64, IN, ReLU                        k_conv7_in on the 8-channel entry tensor, stats, apply
//   model1   two conv 3x3 / stride 2 / zero pad 1 (64 -> 128 -> 256), each IN, ReLU       planner convolutions, stats, apply
//   model2   n residual blocks at 256: x + IN(conv3(reflect 1(ReLU(IN(conv3(reflect 1(x)))))))
//   model3   two ConvTranspose2d 3x3 / stride 2 / pad 1 / output_padding 1 (256 -> 128 -> 64), each IN, ReLU
//   model4   reflect 3, conv 7x7 64 -> 1, optional sigmoid                k_conv7_out, NCHW out
//
// Memory plan.  No padded, shuffled or patched copy of a tensor is made by a pass of its own: the apply pass of the normalisation in
// front of a consumer writes the form that consumer reads (kernels_inorm.hip).
//   - a residual block's input lives ONLY as its pad-1 image: the 3x3 convolutions run on the planner with pad 0 over it (Hi = H + 2,
//     Ho = H), and the block's closing apply pass reads the residual from that image's interior;
//   - a transposed convolution is one linear GEMM, K = 4 Cin, N = 4 Cout, over the 2x2 patch rows the apply pass in front of it wrote,
//     on the weights composed at load (PK_TCONV_SUBPIX); its output stays [H][W][(a, b, Cout)] and both the statistics (which only
//     need every pixel once: 4 H W rows of Cout) and the next apply pass read it in place;
//   - the last apply pass writes the pad-3 image k_conv7_out reads.
// A convolution's bias is kept (the normalisation behind it cancels it in exact arithmetic only).  The planner sees every launch as
// if its sample ran alone (BatchInvariantScope), and the statistics are per-sample partials: a sample's result does not depend on the
// batch it runs in.
#include "model_upscaler.h"

struct gyre_lineart {
    gyre_lineart_cfg cfg;
    Store store;
    Exec ex;
    bool finalized = false;
    UpConv c0, d1, d2, c4;             // model0.1 (7x7), model1.0, model1.3, model4.1 (7x7)
    std::vector<UpConv> rb;            // model2.{i}.conv_block.1 / .5
    UpLin t1, t2;                      // model3.0, model3.3 in sub-pixel form

    void conv3reg(const std::string& key, int cout, int cin, UpConv& c) {
        c.cin = cin; c.cout = cout; c.rows = cout;
        c.w = (bf16_t*)store.dmalloc((size_t)cout * 9 * cin * 2, true);
        store.add(key + ".weight", {cout, cin, 3, 3}, PK_CONV3, c.w, cout, cin);
        c.b = (float*)store.dmalloc((size_t)cout * 4, true);
        store.add(key + ".bias", {cout}, PK_VEC, c.b);
    }
    void conv7reg(const std::string& key, int cout, int cin, int cin_pad, UpConv& c) {
        c.cin = cin_pad; c.cout = cout; c.rows = cout;
        c.w = (bf16_t*)store.dmalloc((size_t)cout * 49 * cin_pad * 2, true);
        store.add(key + ".weight", {cout, cin, 7, 7}, PK_CONV7, c.w, cout, cin_pad);
        c.b = (float*)store.dmalloc((size_t)cout * 4, true);
        store.add(key + ".bias", {cout}, PK_VEC, c.b);
    }
    void tconvreg(const std::string& key, int cin, int cout, UpLin& l) {
        l.K = 4 * cin; l.N = 4 * cout;
        l.w = (bf16_t*)store.dmalloc((size_t)l.N * l.K * 2, true);
        store.add(key + ".weight", {cin, cout, 3, 3}, PK_TCONV_SUBPIX, l.w, l.N, l.K);
        l.b = (float*)store.dmalloc((size_t)l.N * 4, true);
        store.add(key + ".bias", {cout}, PK_VEC_REP4, l.b);
    }
    int build() {
        const gyre_lineart_cfg& c = cfg;
        if (c.input_nc != 3) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "lineart: input_nc 3 is the only one built");
        if (c.output_nc != 1) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "lineart: output_nc 1 is the only one built");
        if (c.n_residual_blocks < 1 || c.n_residual_blocks > 16) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "lineart: 1 to 16 residual blocks are built");
        if (c.sigmoid != 0 && c.sigmoid != 1) GYRE_FAIL(GYRE_ERR_INVALID, "lineart: sigmoid must be 0 or 1");
        ex.store = &store;
        conv7reg("model0.1", 64, 3, 8, c0);
        conv3reg("model1.0", 128, 64, d1);
        conv3reg("model1.3", 256, 128, d2);
        rb.resize(2 * (size_t)c.n_residual_blocks);
        for (int i = 0; i < c.n_residual_blocks; ++i) {
            const std::string p = "model2." + std::to_string(i) + ".conv_block.";
            conv3reg(p + "1", 256, 256, rb[2 * i]);
            conv3reg(p + "5", 256, 256, rb[2 * i + 1]);
        }
        tconvreg("model3.0", 256, 128, t1);
        tconvreg("model3.3", 128, 64, t2);
        conv7reg("model4.1", 1, 64, 64, c4);
        for (void* a : store.allocs) if (!a) GYRE_FAIL(GYRE_ERR_HIP, "hipMalloc failed");
        return 0;
    }

    bf16_t* at(const Tn& t) const { return ex.arena.dry ? (bf16_t*)(uintptr_t)4096 : t.p; }
    // out = conv3x3(x) + bias on the planner: zero padding `pad` (1: the stride-2 convolutions; 0: over a reflect-padded image)
    int conv3(const Tn& x, const UpConv& c, int stride, int pad, Tn& out) {
        const int Ho = (x.H + 2 * pad - 3) / stride + 1, Wo = (x.W + 2 * pad - 3) / stride + 1;
        if (x.C != c.cin || out.C != c.rows || out.H != Ho || out.W != Wo || out.B != x.B) GYRE_FAIL(GYRE_ERR_INVALID, "lineart: internal shape mismatch");
        GemmParams p;
        p.A = at(x); p.lda = x.C; p.mode = GEMM_CONV3;
        p.Hi = x.H; p.Wi = x.W; p.Cin = x.C; p.Ho = Ho; p.Wo = Wo; p.stride = stride; p.pad = pad; p.ups = 0;
        p.W = c.w; p.K = 9 * x.C; p.N = c.rows; p.M = x.B * Ho * Wo;
        p.bias = c.b; p.rows_per_sample = Ho * Wo;
        p.out = at(out); p.ldc = out.C; p.out_mode = OUT_BF16;
        return ex.run_gemm(p);
    }
    // stats of the logical image [B][rows][C] held by t (dense rows of C channels), then the apply pass `a` over it
    int norm(const Tn& t, size_t rows, int C, InormApply a) {
        Tn part, stats;
        TRY(ex.alloc_raw(part, inorm_partial_floats(t.B, rows, C) * sizeof(float)));
        TRY(ex.alloc_raw(stats, (size_t)t.B * C * 2 * sizeof(float)));
        if (!ex.dry()) {
            TRY(launch_inorm_stats(ex.st, t.p, C, t.B, rows, C, 1e-5f, (float*)part.p, (float*)stats.p));
            a.x = t.p; a.stats = (const float*)stats.p; a.B = t.B; a.C = C;
            TRY(launch_inorm_apply(ex.st, a));
        }
        ex.free(part); ex.free(stats);
        return 0;
    }

    int run(bool dry, hipStream_t st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
        if (B < 1 || B > 65535 || H < 5 || W < 5) GYRE_FAIL(GYRE_ERR_INVALID, "lineart: the image must be at least 5 x 5 (below that the reflection paddings have nothing to mirror)");
        if ((size_t)B * H * W > 0x3fffffff) GYRE_FAIL(GYRE_ERR_INVALID, "lineart: image too large");
        BatchInvariantScope invariant;
        ex.arena.reset((char*)ws, wsb, dry); ex.st = st; ex.batch = B; ex.cs_unit = 0;
        const int H1 = (H + 1) / 2, W1 = (W + 1) / 2, H2 = (H1 + 1) / 2, W2 = (W1 + 1) / 2;
        Tn x0, raw, act;
        // model0
        TRY(ex.alloc(x0, B, H, W, 8));
        if (!dry) TRY(launch_nchw_to_nhwc(st, img, idt, B, 3, H * W, 8, x0.p));
        TRY(ex.alloc(raw, B, H, W, 64));
        if (!dry) TRY(launch_conv7_in(st, x0.p, B, H, W, c0.w, c0.b, raw.p));
        ex.free(x0);
        TRY(ex.alloc(act, B, H, W, 64));
        { InormApply a; a.H = H; a.W = W; a.relu = 1; a.out = act.p; TRY(norm(raw, (size_t)H * W, 64, a)); }
        ex.free(raw);
        // model1
        TRY(ex.alloc(raw, B, H1, W1, 128));
        TRY(conv3(act, d1, 2, 1, raw));
        ex.free(act);
        TRY(ex.alloc(act, B, H1, W1, 128));
        { InormApply a; a.H = H1; a.W = W1; a.relu = 1; a.out = act.p; TRY(norm(raw, (size_t)H1 * W1, 128, a)); }
        ex.free(raw);
        TRY(ex.alloc(raw, B, H2, W2, 256));
        TRY(conv3(act, d2, 2, 1, raw));
        ex.free(act);
        // model2: xp = the block input as a pad-1 image, mid = the inner activation likewise
        Tn xp, mid, nxt;
        TRY(ex.alloc(xp, B, H2 + 2, W2 + 2, 256));
        { InormApply a; a.H = H2; a.W = W2; a.relu = 1; a.pad = 1; a.out = xp.p; TRY(norm(raw, (size_t)H2 * W2, 256, a)); }
        TRY(ex.alloc(mid, B, H2 + 2, W2 + 2, 256));
        const int nb = cfg.n_residual_blocks;
        for (int i = 0; i < nb; ++i) {
            TRY(conv3(xp, rb[2 * i], 1, 0, raw));
            { InormApply a; a.H = H2; a.W = W2; a.relu = 1; a.pad = 1; a.out = mid.p; TRY(norm(raw, (size_t)H2 * W2, 256, a)); }
            TRY(conv3(mid, rb[2 * i + 1], 1, 0, raw));
            InormApply a; a.H = H2; a.W = W2; a.res = xp.p; a.res_pad = 1;
            if (i + 1 < nb) { TRY(ex.alloc(nxt, B, H2 + 2, W2 + 2, 256)); a.pad = 1; }
            else { TRY(ex.alloc(nxt, B, H2, W2, 1024)); a.patch = 1; }          // the last block feeds model3.0: 2x2 patch rows
            a.out = nxt.p;
            TRY(norm(raw, (size_t)H2 * W2, 256, a));
            ex.free(xp);
            xp = nxt; nxt = Tn();
        }
        ex.free(mid); ex.free(raw);
        // model3
        Tn up1, pat2, up2, fin;
        TRY(ex.alloc(up1, B, H2, W2, 512));
        TRY(ex.linear(at(xp), 1024, nullptr, 0, 0, xp.rows(), t1.K, t1.w, t1.N, t1.b, nullptr, 0, 0, at(up1), 512));
        ex.free(xp);
        TRY(ex.alloc(pat2, B, 2 * H2, 2 * W2, 512));
        { InormApply a; a.H = 2 * H2; a.W = 2 * W2; a.shuffled = 1; a.relu = 1; a.patch = 1; a.out = pat2.p; TRY(norm(up1, (size_t)4 * H2 * W2, 128, a)); }
        ex.free(up1);
        TRY(ex.alloc(up2, B, 2 * H2, 2 * W2, 256));
        TRY(ex.linear(at(pat2), 512, nullptr, 0, 0, pat2.rows(), t2.K, t2.w, t2.N, t2.b, nullptr, 0, 0, at(up2), 256));
        ex.free(pat2);
        // model4
        const int Ho = 4 * H2, Wo = 4 * W2;
        TRY(ex.alloc(fin, B, Ho + 6, Wo + 6, 64));
        { InormApply a; a.H = Ho; a.W = Wo; a.shuffled = 1; a.relu = 1; a.pad = 3; a.out = fin.p; TRY(norm(up2, (size_t)Ho * Wo, 64, a)); }
        ex.free(up2);
        if (!dry) {
            if (!out) GYRE_FAIL(GYRE_ERR_INVALID, "lineart: null output buffer");
            TRY(launch_conv7_out(st, fin.p, B, Ho, Wo, c4.w, c4.b, cfg.sigmoid, out, odt));
        }
        ex.free(fin);
        return 0;
    }
};

extern "C" {

int gyre_lineart_create(const gyre_lineart_cfg* cfg, int device, gyre_lineart** out) { return handle_create(cfg, device, out); }
void gyre_lineart_destroy(gyre_lineart* h) { delete h; }
int gyre_lineart_num_params(const gyre_lineart* h) { return handle_num_params(h); }
const char* gyre_lineart_param_key(const gyre_lineart* h, int i) { return handle_param_key(h, i); }
int gyre_lineart_set_weight(gyre_lineart* h, const char* key, const void* p, int dtype, const int64_t* shape, int ndim, void* st) {
    return handle_set_weight(h, key, p, dtype, shape, ndim, st);
}
int gyre_lineart_finalize(gyre_lineart* h, void* st) { return handle_finalize(h); }
size_t gyre_lineart_workspace_bytes(gyre_lineart* h, int B, int H, int W) { return handle_workspace_bytes(h, B, H, W); }
int gyre_lineart_forward(gyre_lineart* h, void* st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
    return handle_forward(h, "lineart", st, img, idt, B, H, W, ws, wsb, out, odt);
}

// ---- test hooks of kernels_inorm.hip ----
size_t gyre_op_inorm_workspace(int B, size_t HW, int C) { return inorm_partial_floats(B, HW, C) * sizeof(float); }
int gyre_op_inorm_stats(void* st, const void* x, int ld, int B, size_t HW, int C, float eps, float* partial, float* stats) {
    return launch_inorm_stats((hipStream_t)st, (const bf16_t*)x, ld, B, HW, C, eps, partial, stats);
}
int gyre_op_inorm_apply(void* st, const gyre_inorm_apply_args* g) {
    if (!g) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    InormApply a;
    a.x = (const bf16_t*)g->x; a.stats = g->stats; a.res = (const bf16_t*)g->res; a.out = (bf16_t*)g->out;
    a.B = g->B; a.H = g->H; a.W = g->W; a.C = g->C;
    a.shuffled = g->shuffled; a.relu = g->relu; a.res_pad = g->res_pad; a.pad = g->pad; a.patch = g->patch;
    return launch_inorm_apply((hipStream_t)st, a);
}
int gyre_op_tconv_compose(void* st, const void* w, int dtype, int Cin, int Cout, void* out) {
    return launch_tconv_compose((hipStream_t)st, w, dtype, Cin, Cout, (bf16_t*)out);
}
int gyre_op_conv3x3_valid(void* st, const void* x, int B, int Hi, int Wi, int Cin, const void* w, int Cout, const float* bias, void* y) {
    if (!x || !w || !y) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    if (B < 1 || Hi < 3 || Wi < 3 || Cin < 8 || Cin % 8 || Cout < 8 || Cout % 8 || (size_t)B * Hi * Wi > (1u << 24))
        GYRE_FAIL(GYRE_ERR_INVALID, "conv3x3_valid: an image of at least 3 x 3, Cin and Cout multiples of 8");
    BatchInvariantScope invariant;
    GemmParams p;
    p.A = (const bf16_t*)x; p.lda = Cin; p.mode = GEMM_CONV3;
    p.Hi = Hi; p.Wi = Wi; p.Cin = Cin; p.Ho = Hi - 2; p.Wo = Wi - 2; p.stride = 1; p.pad = 0; p.ups = 0;
    p.W = (const bf16_t*)w; p.K = 9 * Cin; p.N = Cout; p.M = B * p.Ho * p.Wo; p.samples = B;
    p.bias = bias; p.rows_per_sample = p.Ho * p.Wo;
    p.out = y; p.ldc = Cout; p.out_mode = OUT_BF16;
    return launch_gemm((hipStream_t)st, p);
}
int gyre_op_conv7_in(void* st, const void* x8, int B, int H, int W, const void* w, int w_dtype, void* w_scratch, const float* bias, void* out) {
    if (!w || !w_scratch) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    if (w_dtype < 0 || w_dtype > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    if (!x8 || !bias || !out || B < 1 || H < 4 || W < 4) GYRE_FAIL(GYRE_ERR_INVALID, "conv7_in: the image must be at least 4 x 4 (reflection padding 3)");
    TRY(launch_repack_conv((hipStream_t)st, w, w_dtype, 64, 3, 7, 7, 8, (bf16_t*)w_scratch));
    return launch_conv7_in((hipStream_t)st, (const bf16_t*)x8, B, H, W, (const bf16_t*)w_scratch, bias, (bf16_t*)out);
}
int gyre_op_conv7_out(void* st, const void* xp, int B, int Ho, int Wo, const void* w, int w_dtype, void* w_scratch, const float* bias,
                      int sigmoid, void* out, int out_dtype) {
    if (!w || !w_scratch) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    if (w_dtype < 0 || w_dtype > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    if (!xp || !bias || !out || B < 1 || Ho < 1 || Wo < 1) GYRE_FAIL(GYRE_ERR_INVALID, "conv7_out: null argument or empty image");
    TRY(launch_repack_conv((hipStream_t)st, w, w_dtype, 1, 64, 7, 7, 64, (bf16_t*)w_scratch));
    return launch_conv7_out((hipStream_t)st, (const bf16_t*)xp, B, Ho, Wo, (const bf16_t*)w_scratch, bias, sigmoid, out, out_dtype);
}

}  // extern "C"
