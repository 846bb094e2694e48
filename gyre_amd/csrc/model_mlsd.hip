// The MLSD line-detector graph and its C ABI (include/gyre_hip.h): the reference's MobileV2_MLSD_Large (gyre/pipeline/hinters/models/
// mbv2_mlsd_large.py), a MobileNetV2 trunk cut after features[13] and a four-level decoder, whose output feeds the straight-line hint of
// the controlnet/mlsd hintsets.
//
// Topology, every activation NHWC in the storage type at a channel pitch rounded up to 32 (16 -> 32, 24 -> 32, 144 -> 160; the padding
// channels are exactly zero: zero weight rows, zero bias entries, relu6(0) = 0), h = H / 2:
//   entry     NCHW image [B][4][H][W] -> relu6(conv3x3 / 2 + b), [B][h][w][32] (k_mlsd_entry; 4 input channels are below the planner)
//   blocks    13 inverted residuals (t, c, n, s) = (1,16,1,1) (6,24,2,2) (6,32,3,2) (6,64,4,2) (6,96,3,1):
//               expand   1x1 to t c_in channels on the planner, written BEFORE its ReLU6 (absent when t = 1)
//               depthwise 3x3 + b + ReLU6 (k_mlsd_dw), which applies the expand's ReLU6 to what it reads
//               project  1x1 on the planner, no activation; the residual (stride 1, c_in == c_out) rides in its epilogue
//             taps c1 .. c5 after features[1, 3, 6, 10, 13]: 16 ch at h, 24 at h / 2, 32 at h / 4, 64 and 96 at h / 8
//   A blocks  two 1x1 + ReLU branches into one 128-channel concat buffer: a -> channels [0, 64) through the planner's output pixel
//             stride, then k_mlsd_act on that slice; b -> a 64-channel map, then k_mlsd_up2 (ReLU on the reads, bilinear x2
//             align_corners=True) -> channels [64, 128).  block15 does not upsample: both branches write the concat, one ReLU pass.
//   B blocks  planner conv3x3 128 -> 128, k_mlsd_relu_add (relu(y) + x: the ReLU precedes the add), planner conv3x3 128 -> 64, ReLU
//   block23   k_mlsd_dconv (3x3, dilation 5, + b + ReLU), planner conv3x3 + ReLU, planner 1x1 to 16, k_mlsd_exit: x[:, 7:] -> NCHW
// Every BatchNorm is folded at finalize (k_mlsd_fold) from fp32 staging copies of the raw parameters; num_batches_tracked is not a key.
//
// The dilated convolution is a kernel of its own instead of a dilation in the planner's gather: every tile configuration of the planner has its own
// copy of the gather, a new parameter would have to be shown bit-neutral on each, and one 64 -> 64 shape does not pay for that.
//
// Accepted sizes: those where the reference's concatenations line up, n >= 16 and (n / 2) % 8 == 0 per side.
// The planner sees every launch as if its sample ran alone (BatchInvariantScope); the other kernels work per pixel.
#include "model_upscaler.h"

namespace {
constexpr int MLSD_BLOCKS = 13;
struct BlockSpec { int t, cin, cout, stride; };
constexpr BlockSpec MLSD_SPEC[MLSD_BLOCKS] = {
    {1, 32, 16, 1}, {6, 16, 24, 2}, {6, 24, 24, 1}, {6, 24, 32, 2}, {6, 32, 32, 1}, {6, 32, 32, 1}, {6, 32, 64, 2},
    {6, 64, 64, 1}, {6, 64, 64, 1}, {6, 64, 64, 1}, {6, 64, 96, 1}, {6, 96, 96, 1}, {6, 96, 96, 1}};
// features index (block i is features[i + 1]) -> tap number, or -1
inline int tap_of(int feature) { return feature == 1 ? 0 : feature == 3 ? 1 : feature == 6 ? 2 : feature == 10 ? 3 : feature == 13 ? 4 : -1; }
inline bool side_ok(int n) { return n >= 16 && (n / 2) % 8 == 0; }

// a convolution with its BatchNorm: fp32 staging of the raw parameters and the folded result
struct BnConv {
    MlsdFold f;
    bf16_t* w = nullptr; float* bias = nullptr;
};
}  // namespace

struct gyre_mlsd {
    gyre_mlsd_cfg cfg;
    Store store;
    Exec ex;
    bool finalized = false;
    BnConv first, expand[MLSD_BLOCKS], dw[MLSD_BLOCKS], proj[MLSD_BLOCKS];
    BnConv a1[4], a2[4], b1[4], b2[4], c1, c2;              // blocks 15/17/19/21 (conv1, conv2), 16/18/20/22, 23
    UpLin c3;                                               // block23.conv3: biased 1x1 without a BatchNorm
    std::vector<BnConv*> folds;

    float* stage(const std::string& key, std::vector<int64_t> shape) {
        size_t n = 1;
        for (auto d : shape) n *= (size_t)d;
        float* p = (float*)store.dmalloc(n * 4, true);
        store.add(key, std::move(shape), PK_TABLE_F32, p);
        return p;
    }
    // conv: key of the convolution, bn: key of its BatchNorm; state-dict order: conv.weight (conv.bias) bn.weight bn.bias bn.running_mean bn.running_var
    void reg(const std::string& conv, const std::string& bn, int kind, int O, int I, int taps, int o_pad, int i_pad, bool has_bias, BnConv& c) {
        const int k = taps == 9 ? 3 : 1;
        MlsdFold& f = c.f;
        f.kind = kind; f.O = O; f.I = I; f.taps = taps; f.o_pad = o_pad; f.i_pad = i_pad;
        f.w = stage(conv + ".weight", {O, kind == MLSD_FOLD_DEPTHWISE ? 1 : I, k, k});
        if (has_bias) f.conv_bias = stage(conv + ".bias", {O});
        f.gamma = stage(bn + ".weight", {O});
        f.beta = stage(bn + ".bias", {O});
        f.mean = stage(bn + ".running_mean", {O});
        f.var = stage(bn + ".running_var", {O});
        const size_t n = kind == MLSD_FOLD_DENSE ? (size_t)o_pad * taps * i_pad : kind == MLSD_FOLD_DEPTHWISE ? (size_t)9 * o_pad : (size_t)9 * I * o_pad;
        c.w = (bf16_t*)store.dmalloc(n * 2, true);
        c.bias = (float*)store.dmalloc((size_t)o_pad * 4, true);
        f.out = c.w; f.bias = c.bias;
        folds.push_back(&c);
    }
    void dense(const std::string& conv, const std::string& bn, int O, int I, int taps, bool has_bias, BnConv& c) {
        reg(conv, bn, MLSD_FOLD_DENSE, O, I, taps, pad32(O), pad32(I), has_bias, c);
    }
    int build() {
        if (cfg.reserved != 0) GYRE_FAIL(GYRE_ERR_INVALID, "mlsd: the reserved configuration field must be 0");
        ex.store = &store;
        folds.reserve(64);
        reg("backbone.features.0.0", "backbone.features.0.1", MLSD_FOLD_ENTRY, 32, 4, 9, 32, 4, false, first);
        for (int i = 0; i < MLSD_BLOCKS; ++i) {
            const BlockSpec& s = MLSD_SPEC[i];
            const std::string p = "backbone.features." + std::to_string(i + 1) + ".conv.";
            const int hid = s.t * s.cin;
            int n = 0;
            if (s.t != 1) { dense(p + "0.0", p + "0.1", hid, s.cin, 1, false, expand[i]); n = 1; }
            reg(p + std::to_string(n) + ".0", p + std::to_string(n) + ".1", MLSD_FOLD_DEPTHWISE, hid, hid, 9, pad32(hid), pad32(hid), false, dw[i]);
            dense(p + std::to_string(n + 1), p + std::to_string(n + 2), s.cout, hid, 1, false, proj[i]);
        }
        const int a_in1[4] = {64, 32, 24, 16}, a_in2[4] = {96, 64, 64, 64};            // in_c1 (branch a, conv2), in_c2 (branch b, conv1)
        for (int k = 0; k < 4; ++k) {
            const std::string pa = "block" + std::to_string(15 + 2 * k), pb = "block" + std::to_string(16 + 2 * k);
            dense(pa + ".conv1.0", pa + ".conv1.1", 64, a_in2[k], 1, true, a1[k]);
            dense(pa + ".conv2.0", pa + ".conv2.1", 64, a_in1[k], 1, true, a2[k]);
            dense(pb + ".conv1.0", pb + ".conv1.1", 128, 128, 9, true, b1[k]);
            dense(pb + ".conv2.0", pb + ".conv2.1", 64, 128, 9, true, b2[k]);
        }
        dense("block23.conv1.0", "block23.conv1.1", 64, 64, 9, true, c1);
        dense("block23.conv2.0", "block23.conv2.1", 64, 64, 9, true, c2);
        c3.K = 64; c3.N = 16;
        c3.w = (bf16_t*)store.dmalloc((size_t)16 * 64 * 2, true);
        store.add("block23.conv3.weight", {16, 64, 1, 1}, PK_MAT, c3.w, 16, 64);
        c3.b = (float*)store.dmalloc(16 * 4, true);
        store.add("block23.conv3.bias", {16}, PK_VEC, c3.b);
        for (void* a : store.allocs) if (!a) GYRE_FAIL(GYRE_ERR_HIP, "hipMalloc failed");
        return 0;
    }
    int finalize(hipStream_t st) {
        TRY(store.finalize());
        for (const BnConv* c : folds) TRY(launch_mlsd_fold(st, c->f));
        finalized = true;
        return 0;
    }

    bf16_t* at(const Tn& t) const { return ex.arena.dry ? (bf16_t*)(uintptr_t)4096 : t.p; }
    // out[.., 0 .. N) (pixel stride ldc) = x @ w^T + b (+ res), a 1x1 convolution on the planner
    int lin(const Tn& x, const bf16_t* w, const float* b, int K, int N, const Tn* res, bf16_t* out, int ldc) {
        if (x.C != K || (res && res->C != N)) GYRE_FAIL(GYRE_ERR_INVALID, "mlsd: internal shape mismatch");
        return ex.linear(at(x), x.C, nullptr, 0, 0, x.rows(), K, w, N, b, res ? at(*res) : nullptr, res ? res->C : 0, 0, out, ldc);
    }
    int lin(const Tn& x, const BnConv& c, const Tn* res, Tn& out) { return lin(x, c.w, c.bias, c.f.i_pad, c.f.o_pad, res, at(out), out.C); }
    // out = conv3x3(x) + b, zero padding 1, on the planner
    int conv3(const Tn& x, const BnConv& c, Tn& out) {
        if (x.C != c.f.i_pad || out.C != c.f.o_pad || out.H != x.H || out.W != x.W || out.B != x.B) GYRE_FAIL(GYRE_ERR_INVALID, "mlsd: internal shape mismatch");
        GemmParams p;
        p.A = at(x); p.lda = x.C; p.mode = GEMM_CONV3;
        p.Hi = x.H; p.Wi = x.W; p.Cin = x.C; p.Ho = x.H; p.Wo = x.W; p.stride = 1; p.pad = 1; p.ups = 0;
        p.W = c.w; p.K = 9 * x.C; p.N = c.f.o_pad; p.M = x.B * x.H * x.W;
        p.bias = c.bias; p.rows_per_sample = x.H * x.W;
        p.out = at(out); p.ldc = out.C; p.out_mode = OUT_BF16;
        return ex.run_gemm(p);
    }
    int relu(Tn& t) { return ex.dry() ? 0 : launch_mlsd_act(ex.st, t.p, (size_t)t.rows(), t.C, t.C, 0); }

    // BlockTypeA over the taps a (1x1 conv2) and b (1x1 conv1, upsampled x2 unless k == 0) -> cat [B][a.H][a.W][128]
    int block_a(int k, const Tn& a, const Tn& b, Tn& cat) {
        TRY(ex.alloc(cat, a.B, a.H, a.W, 128));
        TRY(lin(a, a2[k].w, a2[k].bias, a2[k].f.i_pad, 64, nullptr, at(cat), 128));
        if (k == 0) {
            TRY(lin(b, a1[k].w, a1[k].bias, a1[k].f.i_pad, 64, nullptr, at(cat) + 64, 128));
            return relu(cat);
        }
        if (a.H != 2 * b.H || a.W != 2 * b.W) GYRE_FAIL(GYRE_ERR_INVALID, "mlsd: internal shape mismatch");
        Tn bb;
        TRY(ex.alloc(bb, b.B, b.H, b.W, 64));
        TRY(lin(b, a1[k], nullptr, bb));
        if (!ex.dry()) {
            TRY(launch_mlsd_act(ex.st, cat.p, (size_t)cat.rows(), 64, 128, 0));
            TRY(launch_mlsd_up2(ex.st, bb.p, b.B, b.H, b.W, 64, 64, 1, cat.p + 64, 128));
        }
        ex.free(bb);
        return 0;
    }
    // BlockTypeB: relu(conv1(x)) + x, then relu(conv2(.)) -> out [..][64]; x is released
    int block_b(int k, Tn& x, Tn& out) {
        Tn t;
        TRY(ex.alloc(t, x.B, x.H, x.W, 128));
        TRY(conv3(x, b1[k], t));
        if (!ex.dry()) TRY(launch_mlsd_relu_add(ex.st, t.p, x.p, (size_t)t.rows() * 128));
        ex.free(x);
        TRY(ex.alloc(out, t.B, t.H, t.W, 64));
        TRY(conv3(t, b2[k], out));
        ex.free(t);
        return relu(out);
    }

    int run(bool dry, hipStream_t st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
        if (B < 1 || B > 65535) GYRE_FAIL(GYRE_ERR_INVALID, "mlsd: a batch of 1 to 65535");
        if (!side_ok(H) || !side_ok(W))
            GYRE_FAIL(GYRE_ERR_INVALID, "mlsd: H and W must be at least 16 with (H / 2) % 8 == 0 and (W / 2) % 8 == 0, got " + std::to_string(H) + " x " + std::to_string(W));
        // the planner indexes rows with 32-bit integers
        if ((size_t)B * (H / 2) * (W / 2) > 0x3fffffff) GYRE_FAIL(GYRE_ERR_INVALID, "mlsd: image too large (B (H / 2) (W / 2) must stay below 2^30)");
        BatchInvariantScope invariant;
        ex.arena.reset((char*)ws, wsb, dry); ex.st = st; ex.batch = B; ex.cs_unit = 0;
        int h = H / 2, w = W / 2;
        Tn cur, c[5];
        TRY(ex.alloc(cur, B, h, w, 32));
        if (!dry) TRY(launch_mlsd_entry(st, img, idt, B, H, W, first.w, first.bias, cur.p));
        for (int i = 0; i < MLSD_BLOCKS; ++i) {
            const BlockSpec& s = MLSD_SPEC[i];
            const int hidp = dw[i].f.o_pad, ho = h / s.stride, wo = w / s.stride;
            const bool res = s.stride == 1 && s.cin == s.cout;
            Tn e, d, o;
            if (s.t != 1) {
                TRY(ex.alloc(e, B, h, w, hidp));
                TRY(lin(cur, expand[i], nullptr, e));
            }
            const Tn& src = s.t != 1 ? e : cur;
            if (src.C != hidp) GYRE_FAIL(GYRE_ERR_INVALID, "mlsd: internal shape mismatch");
            TRY(ex.alloc(d, B, ho, wo, hidp));
            if (!dry) TRY(launch_mlsd_dw(st, src.p, B, h, w, hidp, dw[i].w, dw[i].bias, s.stride, s.t != 1, d.p));
            if (s.t != 1) ex.free(e);
            TRY(ex.alloc(o, B, ho, wo, proj[i].f.o_pad));
            TRY(lin(d, proj[i], res ? &cur : nullptr, o));
            ex.free(d);
            if (tap_of(i) < 0) ex.free(cur);                      // (cur is features[i]; a tap stays until its decoder block)
            cur = o; h = ho; w = wo;
            if (tap_of(i + 1) >= 0) c[tap_of(i + 1)] = cur;
        }
        // decoder: block15 (c4, c5) .. block22
        Tn x, cat;
        TRY(block_a(0, c[3], c[4], cat));
        ex.free(c[3]); ex.free(c[4]);
        TRY(block_b(0, cat, x));
        for (int k = 1; k < 4; ++k) {
            TRY(block_a(k, c[3 - k], x, cat));
            ex.free(c[3 - k]); ex.free(x);
            TRY(block_b(k, cat, x));
        }
        // block23
        Tn t1, t2, t3;
        TRY(ex.alloc(t1, x.B, x.H, x.W, 64));
        if (!dry) TRY(launch_mlsd_dconv(st, x.p, x.B, x.H, x.W, c1.w, c1.bias, t1.p));
        ex.free(x);
        TRY(ex.alloc(t2, t1.B, t1.H, t1.W, 64));
        TRY(conv3(t1, c2, t2));
        ex.free(t1);
        TRY(relu(t2));
        TRY(ex.alloc(t3, t2.B, t2.H, t2.W, 16));
        TRY(lin(t2, c3.w, c3.b, 64, 16, nullptr, at(t3), 16));
        ex.free(t2);
        if (!dry) {
            if (!out) GYRE_FAIL(GYRE_ERR_INVALID, "mlsd: null output buffer");
            TRY(launch_mlsd_exit(st, t3.p, t3.B, t3.H, t3.W, out, odt));
        }
        ex.free(t3);
        return 0;
    }
};

extern "C" {

int gyre_mlsd_create(const gyre_mlsd_cfg* cfg, int device, gyre_mlsd** out) { return handle_create(cfg, device, out); }
void gyre_mlsd_destroy(gyre_mlsd* h) { delete h; }
int gyre_mlsd_num_params(const gyre_mlsd* h) { return handle_num_params(h); }
const char* gyre_mlsd_param_key(const gyre_mlsd* h, int i) { return handle_param_key(h, i); }
int gyre_mlsd_set_weight(gyre_mlsd* h, const char* key, const void* p, int dtype, const int64_t* shape, int ndim, void* st) {
    return handle_set_weight(h, key, p, dtype, shape, ndim, st);
}
int gyre_mlsd_finalize(gyre_mlsd* h, void* st) {
    if (!h) GYRE_FAIL(GYRE_ERR_INVALID, "null handle");
    return h->finalize((hipStream_t)st);
}
size_t gyre_mlsd_workspace_bytes(gyre_mlsd* h, int B, int H, int W) { return handle_workspace_bytes(h, B, H, W); }
int gyre_mlsd_forward(gyre_mlsd* h, void* st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
    return handle_forward(h, "mlsd", st, img, idt, B, H, W, ws, wsb, out, odt);
}

// ---- test hooks of kernels_mlsd.hip ----
int gyre_op_mlsd_fold(void* st, const gyre_mlsd_fold_args* g) {
    if (!g) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    MlsdFold a;
    a.w = g->w; a.conv_bias = g->conv_bias; a.gamma = g->gamma; a.beta = g->beta; a.mean = g->mean; a.var = g->var;
    a.out = (bf16_t*)g->out; a.bias = g->bias; a.kind = g->kind; a.O = g->O; a.I = g->I; a.taps = g->taps; a.o_pad = g->o_pad; a.i_pad = g->i_pad;
    return launch_mlsd_fold((hipStream_t)st, a);
}
int gyre_op_mlsd_entry(void* st, const void* x, int dtype, int B, int H, int W, const void* w, const float* bias, void* y) {
    return launch_mlsd_entry((hipStream_t)st, x, dtype, B, H, W, (const bf16_t*)w, bias, (bf16_t*)y);
}
int gyre_op_dwconv3(void* st, const void* x, int B, int H, int W, int C, const void* w, const float* bias, int stride, int relu6_in, void* y) {
    return launch_mlsd_dw((hipStream_t)st, (const bf16_t*)x, B, H, W, C, (const bf16_t*)w, bias, stride, relu6_in, (bf16_t*)y);
}
int gyre_op_upsample2_ac(void* st, const void* x, int B, int H, int W, int C, int ldx, int relu_in, void* y, int ldy) {
    return launch_mlsd_up2((hipStream_t)st, (const bf16_t*)x, B, H, W, C, ldx, relu_in, (bf16_t*)y, ldy);
}
int gyre_op_dconv3_d5(void* st, const void* x, int B, int H, int W, const void* w, const float* bias, void* y) {
    return launch_mlsd_dconv((hipStream_t)st, (const bf16_t*)x, B, H, W, (const bf16_t*)w, bias, (bf16_t*)y);
}
int gyre_op_mlsd_act(void* st, void* x, size_t rows, int C, int ld, int relu6) {
    return launch_mlsd_act((hipStream_t)st, (bf16_t*)x, rows, C, ld, relu6);
}
int gyre_op_mlsd_relu_add(void* st, void* y, const void* x, size_t n) {
    return launch_mlsd_relu_add((hipStream_t)st, (bf16_t*)y, (const bf16_t*)x, n);
}
int gyre_op_mlsd_exit(void* st, const void* x, int B, int H, int W, void* out, int out_dtype) {
    return launch_mlsd_exit((hipStream_t)st, (const bf16_t*)x, B, H, W, out, out_dtype);
}

}  // extern "C"
