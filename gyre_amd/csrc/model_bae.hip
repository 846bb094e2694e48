// The decoder of the BAE surface-normal estimator and its C ABI (include/gyre_hip.h): the reference's Decoder (gyre/pipeline/hinters/
// baenormal/submodules/decoder.py) with architecture 'BN' in mode='test', whose last map feeds the normal-map hint of the
// controlnet/normalbae hintsets.  The EfficientNet-B5 encoder in front of it (about 3 % of the network's arithmetic) stays the host module
// the caller supplies; the handle takes its five feature maps.
//
// Topology, every activation NHWC in the storage type, NF = num_features, (h_k, w_k) the size of x_block_k (h_(k+1) = ceil(h_k / 2)):
//   entry     x_block4 NCHW -> NHWC [B][h4][w4][NF] (k_bae_up_concat with nothing to resize)
//   conv2     1x1 NF -> NF on the planner: x_d0
//   up K      (K = 1 .. 4, UpSampleBN) k_bae_up_concat: bilinear resize of x_d(K-1) to the size of x_block(4-K) | that skip map | zeros up
//             to a channel pitch rounded up to 32 (2224 -> 2240, 1088, 552 -> 576, 280 -> 288; the padded weight columns are zero);
//             two planner conv3x3 with their BatchNorms folded, each followed by LeakyReLU(0.01) in place (launch_swin_act): x_dK at
//             NF / 2, / 4, / 8, / 16 channels
//   res8      planner conv3x3 NF / 4 -> 4 (32 weight rows) on x_d2, k_bae_norm8: out_res8, NCHW fp32
//   res4/2/1  ONE k_bae_refine launch each on (x_d2, out_res8), (x_d3, out_res4), (x_d4, out_res2): bilinear x2, the four-layer per-pixel
//             MLP and norm_normalize fused (kernels_bae.hip); the predictions stay fp32 between the stages
//   exit      the four maps cast to the caller's dtype, back to back
// finalize folds every BatchNorm into its convolution (k_mlsd_fold: fp32 from fp32 staging copies of the raw parameters, one rounding).
// Accepted sizes: h0 % 4 == 0 and w0 % 4 == 0 - the reference's torch.cat in the res2 / res1 stages needs x_block1 = 2 x_block2 and
// x_block0 = 2 x_block1.  The planner sees every launch as if its sample ran alone (BatchInvariantScope); the other kernels work per
// pixel or tile.  The weight registration, the planner calls with their shape checks and the C ABI shell are ImageGraph's.
#include "model_upscaler.h"

namespace {
// a 3x3 convolution with its BatchNorm: fp32 staging of the raw parameters and the folded result
struct BaeBnConv {
    MlsdFold f;
    bf16_t* w = nullptr; float* bias = nullptr;
    UpConv conv() const { UpConv c; c.w = w; c.b = bias; c.cin = f.i_pad; c.cout = f.O; c.rows = f.o_pad; return c; }
};
// a refinement stage's four Conv1d layers
struct BaeMlp { int CF = 0; bf16_t *w1, *w2, *w3; float *b1, *b2, *b3, *w4, *b4; };
inline int half_up(int n) { return (n + 1) / 2; }
}  // namespace

struct gyre_bae : ImageGraph {
    gyre_bae_cfg cfg;
    UpLin conv2;
    BaeBnConv up[4][2];
    UpConv res8;
    BaeMlp mlp[3];
    int cs[5] = {0, 0, 0, 0, 0};                            // channels of x_block0 .. x_block4
    gyre_bae() : ImageGraph("bae") {}

    // state-dict order: conv.weight conv.bias bn.weight bn.bias bn.running_mean bn.running_var
    void bn_conv(const std::string& conv, const std::string& bn, int O, int I, BaeBnConv& c) {
        MlsdFold& f = c.f;
        f.kind = MLSD_FOLD_DENSE; f.O = O; f.I = I; f.taps = 9; f.o_pad = pad32(O); f.i_pad = pad32(I);
        f.w = f32(conv + ".weight", {O, I, 3, 3});
        f.conv_bias = f32(conv + ".bias", {O});
        f.gamma = f32(bn + ".weight", {O});
        f.beta = f32(bn + ".bias", {O});
        f.mean = f32(bn + ".running_mean", {O});
        f.var = f32(bn + ".running_var", {O});
        c.w = (bf16_t*)store.dmalloc((size_t)f.o_pad * 9 * f.i_pad * 2, true);
        c.bias = (float*)store.dmalloc((size_t)f.o_pad * 4, true);
        f.out = c.w; f.bias = c.bias;
    }
    // nn.Conv1d(I, O, 1): weight [O][I][1] as a matrix [O][ipad] in storage, bias fp32
    void conv1d(const std::string& key, int O, int I, int ipad, bf16_t** w, float** b) {
        *w = (bf16_t*)store.dmalloc((size_t)O * ipad * 2, true);
        store.add(key + ".weight", {O, I, 1}, PK_MAT, *w, O, ipad);
        store.vec(key + ".bias", O, b);
    }
    int build() {
        const int NF = cfg.num_features;
        if (cfg.architecture != 0) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "bae: architecture 'BN' is the form built ('GN': weight standardisation + GroupNorm is not)");
        if (NF < 512 || NF % 512 || NF > 4096) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "bae: num_features must be a multiple of 512, 512 to 4096");
        for (int k = 0; k < 4; ++k) {
            if (cfg.skip[k] < 1 || cfg.skip[k] > 4096) GYRE_FAIL(GYRE_ERR_INVALID, "bae: skip widths of 1 to 4096 channels");
            cs[k] = cfg.skip[k];
        }
        cs[4] = NF;
        lin("conv2", NF, NF, NF, NF, true, true, conv2);
        for (int k = 0; k < 4; ++k) {
            const std::string p = "up" + std::to_string(k + 1) + "._net.";
            const int cin = (NF >> k) + cs[3 - k], cout = NF >> (k + 1);
            bn_conv(p + "0", p + "1", cout, cin, up[k][0]);
            bn_conv(p + "3", p + "4", cout, cout, up[k][1]);
        }
        conv("out_conv_res8", 4, NF / 4, 3, 32, NF / 4, PK_CONV3, res8);
        const char* names[3] = {"out_conv_res4.", "out_conv_res2.", "out_conv_res1."};
        for (int s = 0; s < 3; ++s) {
            BaeMlp& m = mlp[s];
            const std::string p = names[s];
            m.CF = NF >> (s + 2);
            conv1d(p + "0", 128, m.CF + 4, m.CF + 32, &m.w1, &m.b1);
            conv1d(p + "2", 128, 128, 128, &m.w2, &m.b2);
            conv1d(p + "4", 128, 128, 128, &m.w3, &m.b3);
            m.w4 = f32(p + "6.weight", {4, 128, 1});
            store.vec(p + "6.bias", 4, &m.b4);
        }
        return check_allocs();
    }
    int finalize(hipStream_t st) {
        TRY(store.finalize());
        for (int k = 0; k < 4; ++k)
            for (int j = 0; j < 2; ++j) TRY(launch_mlsd_fold(st, up[k][j].f));
        finalized = true;
        return 0;
    }

    // out = leaky_relu_0.01(BN(conv3x3(x))), zero padding 1
    int conv_bn_act(const Tn& x, const BaeBnConv& c, Tn& out) {
        TRY(ex.alloc(out, x.B, x.H, x.W, c.f.o_pad));
        TRY(conv3(x, x.C, c.conv(), 1, 1, 0, nullptr, out));
        return ex.dry() ? 0 : launch_swin_act(ex.st, out.p, (size_t)out.rows() * out.C, 1, 0.01f);
    }
    // a refinement stage: (x, pred at x's size) -> fine, fp32 NCHW at twice the size
    int refine(const BaeMlp& m, const Tn& x, const Tn& pred, Tn& fine) {
        if (x.C != m.CF) return mismatch();
        TRY(ex.alloc(fine, x.B, 4, 2 * x.H, 2 * x.W, 4));                  // (NCHW fp32: four planes, 4-byte elements)
        if (ex.dry()) return 0;
        return launch_bae_refine(ex.st, x.p, x.C, (const float*)pred.p, x.B, x.H, x.W, m.CF, m.w1, m.b1, m.w2, m.b2, m.w3, m.b3, m.w4, m.b4, 1,
                                 (float*)fine.p);
    }

    // img: x_block0 .. x_block4 back to back, NCHW of idt; H, W: the size of x_block0
    int run(bool dry, hipStream_t st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
        if (B < 1 || B > 65535) GYRE_FAIL(GYRE_ERR_INVALID, "bae: a batch of 1 to 65535");
        if (H < 4 || W < 4 || H % 4 || W % 4)
            GYRE_FAIL(GYRE_ERR_INVALID, "bae: the sides of x_block0 must be positive multiples of 4 (the reference's concatenations line up at no other size), got " +
                                        std::to_string(H) + " x " + std::to_string(W));
        // the planner indexes elements with 32-bit integers; the largest tensor is up4's concat at the size of x_block0
        if ((size_t)B * H * W > 0x3fffffff / (size_t)up[3][0].f.i_pad) GYRE_FAIL(GYRE_ERR_INVALID, "bae: image too large");
        if (!dry && !out) GYRE_FAIL(GYRE_ERR_INVALID, "bae: null output buffer");
        int h[5], w[5];
        size_t at_[5], ofs = 0;
        const size_t isz = idt == 0 ? 4 : 2;
        for (int k = 0; k < 5; ++k) {
            h[k] = k ? half_up(h[k - 1]) : H; w[k] = k ? half_up(w[k - 1]) : W;
            at_[k] = ofs;
            ofs += (size_t)B * cs[k] * h[k] * w[k] * isz;
        }
        BatchInvariantScope invariant;
        begin(dry, st, B, ws, wsb);
        const int NF = cfg.num_features;
        Tn e, d, keep[3];                                                   // keep: x_d2, x_d3, x_d4
        TRY(ex.alloc(e, B, h[4], w[4], NF));
        if (!dry) TRY(launch_bae_up_concat(st, nullptr, B, 0, 0, 0, 0, (const char*)img + at_[4], idt, NF, h[4], w[4], e.p, NF));
        TRY(ex.alloc(d, B, h[4], w[4], NF));
        TRY(linear(e, conv2, nullptr, d));
        ex.free(e);
        for (int k = 0; k < 4; ++k) {
            const int sk = 3 - k, C = NF >> k;
            Tn cat, a, o;
            TRY(ex.alloc(cat, B, h[sk], w[sk], up[k][0].f.i_pad));
            if (!dry) TRY(launch_bae_up_concat(st, d.p, B, d.H, d.W, C, d.C, (const char*)img + at_[sk], idt, cs[sk], h[sk], w[sk], cat.p, cat.C));
            if (k < 2) ex.free(d);                                          // (x_d2 and x_d3 stay for their refinement stages)
            TRY(conv_bn_act(cat, up[k][0], a));
            ex.free(cat);
            TRY(conv_bn_act(a, up[k][1], o));
            ex.free(a);
            d = o;
            if (k >= 1) keep[k - 1] = o;
        }
        // out_res8 and the three refinement stages
        Tn r8, pr[4];
        TRY(ex.alloc(r8, B, h[2], w[2], 32));
        TRY(conv3(keep[0], keep[0].C, res8, 1, 1, 0, nullptr, r8));
        TRY(ex.alloc(pr[0], B, 4, h[2], w[2], 4));
        if (!dry) TRY(launch_bae_norm8(st, r8.p, 32, B, (size_t)h[2] * w[2], (float*)pr[0].p));
        ex.free(r8);
        for (int s = 0; s < 3; ++s) {
            TRY(refine(mlp[s], keep[s], pr[s], pr[s + 1]));
            ex.free(keep[s]);
        }
        const size_t osz = odt == 0 ? 4 : 2;
        char* op = (char*)out;
        for (int s = 0; s < 4; ++s) {
            const size_t n = (size_t)B * 4 * (h[2] << s) * (w[2] << s);
            if (!dry) TRY(launch_bae_exit(st, (const float*)pr[s].p, n, op, odt));
            op += n * osz;
            ex.free(pr[s]);
        }
        return 0;
    }
};

GYRE_IMAGE_MODEL_ABI(bae)

extern "C" {

// ---- test hooks of kernels_bae.hip ----
int gyre_op_bae_refine(void* st, const void* x, int ldx, const float* pred, int B, int Hs, int Ws, int CF, const void* w1, const float* b1,
                       const void* w2, const float* b2, const void* w3, const float* b3, const float* w4, const float* b4, int normalize,
                       float* out) {
    return launch_bae_refine((hipStream_t)st, (const bf16_t*)x, ldx, pred, B, Hs, Ws, CF, (const bf16_t*)w1, b1, (const bf16_t*)w2, b2,
                             (const bf16_t*)w3, b3, w4, b4, normalize, out);
}
int gyre_op_bae_refine_tile(int32_t* rows, int32_t* cols) {
    if (!rows || !cols) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    int th, tw;
    bae_refine_tile(&th, &tw);
    *rows = th; *cols = tw;
    return 0;
}
int gyre_op_bae_up_concat(void* st, const void* x, int B, int Hs, int Ws, int C, int ldx, const void* skip, int skip_dtype, int Cs, int H,
                          int W, void* y, int ldo) {
    return launch_bae_up_concat((hipStream_t)st, (const bf16_t*)x, B, Hs, Ws, C, ldx, skip, skip_dtype, Cs, H, W, (bf16_t*)y, ldo);
}

}  // extern "C"
