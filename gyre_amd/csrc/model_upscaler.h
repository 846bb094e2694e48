// What the image-in / image-out graphs share: the weight records, ImageGraph - the base of all eight graphs, described below - and
// WinTrunk, everything of a window-transformer upscaler (SwinIR, HAT) that is not its attention launch, its extra branches or its
// upsampler tail.
//
// Memory plan of the trunk.  Tokens stay in image order, NHWC with Cp = embed_dim rounded up to 32 channels (180 -> 192, 240 -> 256); the
// padding channels are exactly zero everywhere: zero weight rows and bias entries in every producer, zeros written by the LayerNorm, and
// the attention output buffer - whose padding columns the kernels never write - is cleared once per call.  The qkv projection writes
// 32-column groups per (q | k | v, head) (PK_MAT_HEAD30); the attention kernels read them through the window map, so no rolled or
// partitioned copy exists.  Three Cp-channel tensors rotate through a residual group: its input (kept for the closing residual) and the
// two the blocks alternate between.
//
// Kernels.  Every GEMM and convolution goes through the planner (Exec::run_gemm); residual additions ride in the GEMM epilogues.  The
// LayerNorms are the stand-alone launch_ln_live: the planner's folded form takes its statistics over the whole K = Cp row, which is not
// the live-channel mean, so the fold does not apply to a padded width.  GELU and the leaky ReLUs are in-place passes (launch_swin_act).
//
// Three orders are part of the behaviour and every helper here keeps them: store.add (the index order of gyre_*_param_key), ex.alloc /
// ex.free (the arena offsets and workspace_bytes), and the launches (gyre_last_launch_count and, through split-K planning, the bits).
//
// ImageGraph is the base of every image-in / image-out graph (model_rrdb, _swinir, _hat, _lineart, _hed, _mlsd, _swinb, _uniformer.hip):
// the handle members the handle_* templates of model_impl.h read, the registration of a weight with its bias, the planner calls with
// their shape checks and the dry-run stand-in pointer.  GYRE_IMAGE_MODEL_ABI(kind) emits a family's eight C entry points.  What differs
// between families stays with them: the LayerNorm launcher and eps, the activation passes, whether run() takes a BatchInvariantScope
// (gyre_rrdb does not), which derived buffers are zero-filled, the size refusals.
#pragma once
#include "model_impl.h"

struct UpConv { bf16_t* w = nullptr; float* b = nullptr; int cin = 0, cout = 0, rows = 0; };   // cin / rows: padded input channels / weight rows
struct UpLin { bf16_t* w = nullptr; float* b = nullptr; int K = 0, N = 0; };                   // padded
struct Bn { float *g, *b, *m, *v; };                                                           // weight, bias, running_mean, running_var
// what a SwinIR block, a HAB and an OCAB each own: two norms, the position table, qkv and proj, the MLP
struct WinAttnW { float *g1, *b1, *g2, *b2, *table; UpLin qkv, proj, fc1, fc2; };
static inline int pad32(int c) { return (c + 31) / 32 * 32; }

// The planner sees every launch as if its sample ran alone - no batch-dependent split-K factor - while one of these is alive
struct BatchInvariantScope {
    const int prev = gemm_set_batch_invariant(1);
    ~BatchInvariantScope() { gemm_set_batch_invariant(prev); }
};

struct ImageGraph {
    const char* const name;        // "swinir", "hed", ...: the prefix of every refusal
    Store store;
    Exec ex;
    bool finalized = false;
    explicit ImageGraph(const char* n) : name(n) { ex.store = &store; }

    // ---- registration: every helper adds its keys in state-dict order (.weight, then .bias) ----
    // a k x k convolution as rows x (k k cin_pad), pack PK_CONV3 / PK_CONV7; the rows above cout and the channels above cin stay zero
    void conv(const std::string& key, int cout, int cin, int k, int rows, int cin_pad, int pack, UpConv& c) {
        c.cin = cin_pad; c.cout = cout; c.rows = rows;
        c.w = (bf16_t*)store.dmalloc((size_t)rows * k * k * cin_pad * 2, true);
        store.add(key + ".weight", {cout, cin, k, k}, pack, c.w, rows, cin_pad);
        c.b = (float*)store.dmalloc((size_t)rows * 4, true);
        store.add(key + ".bias", {cout}, PK_VEC, c.b);
    }
    // nn.Linear, or a 1x1 convolution (conv1x1: the key's shape has the two trailing ones), as rows x ipad
    void lin(const std::string& key, int O, int I, int rows, int ipad, bool has_bias, bool conv1x1, UpLin& l) {
        l.K = ipad; l.N = rows;
        l.w = (bf16_t*)store.dmalloc((size_t)rows * ipad * 2, true);
        store.add(key + ".weight", conv1x1 ? std::vector<int64_t>{O, I, 1, 1} : std::vector<int64_t>{O, I}, PK_MAT, l.w, rows, ipad);
        if (!has_bias) return;
        l.b = (float*)store.dmalloc((size_t)rows * 4, true);
        store.add(key + ".bias", {O}, PK_VEC, l.b);
    }
    void norm(const std::string& key, int C, float** g, float** b) {
        store.vec(key + ".weight", C, g);
        store.vec(key + ".bias", C, b);
    }
    void bnorm(const std::string& key, int C, Bn& n) {
        norm(key, C, &n.g, &n.b);
        store.vec(key + ".running_mean", C, &n.m);
        store.vec(key + ".running_var", C, &n.v);
    }
    // a tensor kept in fp32 as it is stored: tables, staging copies of weights a finalize step folds
    float* f32(const std::string& key, std::vector<int64_t> shape) {
        size_t n = 1;
        for (auto d : shape) n *= (size_t)d;
        float* p = (float*)store.dmalloc(n * 4, true);
        store.add(key, std::move(shape), PK_TABLE_F32, p);
        return p;
    }
    int check_allocs() const {
        for (void* a : store.allocs) if (!a) GYRE_FAIL(GYRE_ERR_HIP, "hipMalloc failed");
        return 0;
    }
    // what a family without derived weights needs; one with them hides this with its own
    int finalize(hipStream_t) {
        TRY(store.finalize());
        finalized = true;
        return 0;
    }

    // ---- execution ----
    int mismatch() const { GYRE_FAIL(GYRE_ERR_INVALID, std::string(name) + ": internal shape mismatch"); }
    void begin(bool dry, hipStream_t st, int B, void* ws, size_t wsb) {
        ex.arena.reset((char*)ws, wsb, dry); ex.st = st; ex.batch = B; ex.cs_unit = 0;
    }
    // channel c0 of t; a dry run plans with aligned stand-ins of the same residue mod 256 (arena tensors are 256-byte aligned)
    bf16_t* at(const Tn& t, int c0 = 0) const { return ex.arena.dry ? (bf16_t*)(uintptr_t)(4096 + 2 * c0) : t.p + c0; }
    // out[pix][c0 .. c0 + c.rows) = conv3x3(x[pix][0 .. Cin)) + bias (+ res), zero padding `pad`; ups: nearest 2x inside the gather
    // (stride 1, pad 1).  The plain planner convolution: the caller owns `out`, no column statistics, no four-parity form
    int conv3(const Tn& x, int Cin, const UpConv& c, int stride, int pad, int ups, const Tn* res, Tn& out, int c0 = 0) {
        const int Ho = ups ? 2 * x.H : (x.H + 2 * pad - 3) / stride + 1, Wo = ups ? 2 * x.W : (x.W + 2 * pad - 3) / stride + 1;
        if (Cin != c.cin || Cin > x.C || c0 + c.rows > out.C || out.H != Ho || out.W != Wo || out.B != x.B || (res && res->C != c.rows)) return mismatch();
        GemmParams p;
        p.A = at(x); p.lda = x.C; p.mode = GEMM_CONV3;
        p.Hi = x.H; p.Wi = x.W; p.Cin = Cin; p.Ho = Ho; p.Wo = Wo; p.stride = stride; p.pad = pad; p.ups = ups;
        p.Hup = ups ? Ho : 0; p.Wup = ups ? Wo : 0;
        p.W = c.w; p.K = 9 * Cin; p.N = c.rows; p.M = x.B * Ho * Wo;
        p.bias = c.b; p.rows_per_sample = Ho * Wo;
        if (res) { p.residual = at(*res); p.ldr = res->C; }
        p.out = at(out, c0); p.ldc = out.C; p.out_mode = OUT_BF16;
        return ex.run_gemm(p);
    }
    // out[.., 0 .. N) (row stride ldc) = x @ w^T + b (+ res): a linear or 1x1 convolution into a slice of a wider tensor
    int linear_to(const Tn& x, const bf16_t* w, const float* b, int K, int N, const Tn* res, bf16_t* out, int ldc) {
        if (x.C != K || (res && res->C != N)) return mismatch();
        return ex.linear(at(x), x.C, nullptr, 0, 0, x.rows(), K, w, N, b, res ? at(*res) : nullptr, res ? res->C : 0, 0, out, ldc);
    }
    int linear(const Tn& x, const UpLin& l, const Tn* res, Tn& out) {
        if (out.C != l.N) return mismatch();
        return linear_to(x, l.w, l.b, l.K, l.N, res, at(out), out.C);
    }
};

// The C entry points every image model has (include/gyre_hip.h), on the handle_* bodies of model_impl.h
#define GYRE_IMAGE_MODEL_ABI(kind)                                                                                                          \
    extern "C" {                                                                                                                            \
    int gyre_##kind##_create(const gyre_##kind##_cfg* cfg, int device, gyre_##kind** out) { return handle_create(cfg, device, out); }       \
    void gyre_##kind##_destroy(gyre_##kind* h) { delete h; }                                                                                \
    int gyre_##kind##_num_params(const gyre_##kind* h) { return handle_num_params(h); }                                                     \
    const char* gyre_##kind##_param_key(const gyre_##kind* h, int i) { return handle_param_key(h, i); }                                     \
    int gyre_##kind##_set_weight(gyre_##kind* h, const char* key, const void* p, int dtype, const int64_t* shape, int ndim, void* st) {     \
        return handle_set_weight(h, key, p, dtype, shape, ndim, st);                                                                        \
    }                                                                                                                                       \
    int gyre_##kind##_finalize(gyre_##kind* h, void* st) { return handle_finalize(h, st); }                                                 \
    size_t gyre_##kind##_workspace_bytes(gyre_##kind* h, int B, int H, int W) { return handle_workspace_bytes(h, B, H, W); }                \
    int gyre_##kind##_forward(gyre_##kind* h, void* st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out,     \
                              int odt) {                                                                                                    \
        return handle_forward(h, #kind, st, img, idt, B, H, W, ws, wsb, out, odt);                                                          \
    }                                                                                                                                       \
    }

struct WinTrunk : ImageGraph {
    int C = 0, Cp = 0, heads = 0, hid = 0;
    float mean[3] = {0.4488f, 0.4371f, 0.4040f}, img_range = 1.f;
    UpConv conv_first, conv_bu, conv_last;
    float *pe_g = nullptr, *pe_b = nullptr, *n_g = nullptr, *n_b = nullptr;
    using ImageGraph::ImageGraph;
    using ImageGraph::conv3;

    // ---- registration of the trunk's own shapes ----
    void conv(const std::string& key, int cout, int cin, int rows, int cin_pad, UpConv& c) { ImageGraph::conv(key, cout, cin, 3, rows, cin_pad, PK_CONV3, c); }
    void lin(const std::string& key, int O, int I, int rows, int ipad, UpLin& l, bool conv1x1 = false) { ImageGraph::lin(key, O, I, rows, ipad, true, conv1x1, l); }
    void norm(const std::string& key, float** g, float** b) { ImageGraph::norm(key, C, g, b); }
    void table(const std::string& key, int rows, WinAttnW& a) { a.table = f32(key, {rows, heads}); }
    // qkv and proj under p (".attn" of a block, the OCAB itself)
    void qkv_proj(const std::string& p, WinAttnW& a) {
        a.qkv.K = Cp; a.qkv.N = 96 * heads;
        a.qkv.w = (bf16_t*)store.dmalloc((size_t)a.qkv.N * Cp * 2, true);
        store.add(p + ".qkv.weight", {3 * C, C}, PK_MAT_HEAD30, a.qkv.w, a.qkv.N, Cp);
        a.qkv.b = (float*)store.dmalloc((size_t)a.qkv.N * 4, true);
        store.add(p + ".qkv.bias", {3 * C}, PK_VEC_HEAD30, a.qkv.b);
        lin(p + ".proj", C, C, Cp, Cp, a.proj);
    }
    // a block's norm1, attn.relative_position_bias_table (table_rows: 225 at window 8, 961 at 16), attn.qkv, attn.proj
    void block_attn(const std::string& p, int table_rows, WinAttnW& a) {
        norm(p + ".norm1", &a.g1, &a.b1);
        table(p + ".attn.relative_position_bias_table", table_rows, a);
        qkv_proj(p + ".attn", a);
    }
    void mlp(const std::string& p, WinAttnW& a) {
        norm(p + ".norm2", &a.g2, &a.b2);
        lin(p + ".mlp.fc1", hid, C, hid, Cp, a.fc1);
        lin(p + ".mlp.fc2", C, hid, Cp, hid, a.fc2);
    }
    // The refusals both families share, then the widths and the head of the state dict (conv_first, patch_embed.norm).  The cfg structs
    // carry the same field names; upsampler: the one form the family builds
    template <typename Cfg> int configure(const Cfg& c, const char* upsampler) {
        const std::string n = std::string(name) + ": ";
        if (c.in_chans != 3) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, n + "in_chans 3 is the only one built");
        if (c.upscale != 2 && c.upscale != 4) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, n + upsampler + " with upscale 2 or 4 is built");
        if (c.num_layers < 1 || c.num_layers > 16) GYRE_FAIL(GYRE_ERR_INVALID, n + "1 to 16 layers");
        heads = c.num_heads[0];
        for (int i = 0; i < c.num_layers; ++i) {
            if (c.num_heads[i] != heads) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, n + "the same head count in every layer is built");
            if (c.depths[i] < 1 || c.depths[i] > 64) GYRE_FAIL(GYRE_ERR_INVALID, n + "depth out of range");
        }
        if (heads < 1 || heads > 8 || c.embed_dim != 30 * heads) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, n + "embed_dim = 30 * heads with at most 8 heads is built");
        if (c.mlp_hidden < 8 || c.mlp_hidden % 8) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, n + "the MLP width must be a multiple of 8");
        if (!(c.img_range > 0.f)) GYRE_FAIL(GYRE_ERR_INVALID, n + "img_range must be positive");
        C = c.embed_dim; Cp = pad32(C); hid = c.mlp_hidden; img_range = c.img_range;
        conv("conv_first", C, 3, Cp, 8, conv_first);
        norm("patch_embed.norm", &pe_g, &pe_b);
        return 0;
    }

    // ---- execution ----
    // the trunk's convolutions: a whole tensor in, a whole tensor out, stride 1, padding 1
    int conv3(const Tn& x, const UpConv& c, int ups, const Tn* res, Tn& out) {
        if (out.C != c.rows) return mismatch();
        return conv3(x, x.C, c, 1, 1, ups, res, out);
    }
    int act(Tn& t, int mode, float slope) {
        if (ex.dry()) return 0;
        return launch_swin_act(ex.st, t.p, (size_t)t.rows() * t.C, mode, slope);
    }
    int ln(const Tn& x, const float* g, const float* b, Tn& y) {
        if (ex.dry()) return 0;
        return launch_ln_live(ex.st, x.p, x.C, (size_t)x.rows(), C, g, b, 1e-5f, y.p, y.C);
    }

    // The tensors of a call: conv_first's output, the three that rotate through a residual group (rin: the group's input, u / v: the
    // two its blocks alternate between) and the scratch of a block
    struct Bufs {
        Tn feat, a, t1, t2, nrm, qkv, ao, hdn;
        Tn *rin = &a, *u = &t1, *v = &t2;
    };
    // entry kernel, conv_first, the allocations, patch_embed.norm -> *w.rin
    int head(bool dry, hipStream_t st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, int window, Bufs& w) {
        if (B < 1 || H < window || W < window || H % window || W % window)
            GYRE_FAIL(GYRE_ERR_INVALID, std::string(name) + ": H and W must be positive multiples of the window size " + std::to_string(window));
        begin(dry, st, B, ws, wsb);
        Tn x0;
        TRY(ex.alloc(x0, B, H, W, 8));
        if (!dry) TRY(launch_swin_entry(st, img, idt, B, (size_t)H * W, mean, img_range, x0.p));
        TRY(ex.alloc(w.feat, B, H, W, Cp));
        TRY(conv3(x0, conv_first, 0, nullptr, w.feat));
        ex.free(x0);
        TRY(ex.alloc(w.a, B, H, W, Cp));
        TRY(ex.alloc(w.t1, B, H, W, Cp));
        TRY(ex.alloc(w.t2, B, H, W, Cp));
        TRY(ex.alloc(w.nrm, B, H, W, Cp));
        TRY(ex.alloc(w.qkv, B, H, W, 96 * heads));
        TRY(ex.alloc(w.ao, B, H, W, Cp));
        TRY(ex.alloc(w.hdn, B, H, W, hid));
        if (!dry) GYRE_HIP_CHECK(hipMemsetAsync(w.ao.p, 0, w.ao.bytes, st));     // the padding columns [C, Cp) stay zero: the kernel never writes them
        return ln(w.feat, pe_g, pe_b, w.a);
    }
    // u = x + proj(attn(qkv(LN1(x)))); leaves LN1(x) in w.nrm.  attn(): the model's own launch from w.qkv into w.ao, not called in a dry run
    template <typename F> int attn_part(const WinAttnW& a, const Tn& x, Bufs& w, Tn& u, F&& attn) {
        TRY(ln(x, a.g1, a.b1, w.nrm));
        TRY(linear(w.nrm, a.qkv, nullptr, w.qkv));
        if (!ex.dry()) TRY(attn());
        return linear(w.ao, a.proj, &x, u);
    }
    // v = u + fc2(gelu(fc1(LN2(u))))
    int mlp_part(const WinAttnW& a, Tn& u, Bufs& w, Tn& v) {
        TRY(ln(u, a.g2, a.b2, w.nrm));
        TRY(linear(w.nrm, a.fc1, nullptr, w.hdn));
        TRY(act(w.hdn, 0, 0.f));
        return linear(w.hdn, a.fc2, &u, v);
    }
    // w.nrm = norm(body); the block scratch is released.  conv_after_body(w.nrm) + w.feat -> *w.u is the model's
    int final_norm(Bufs& w) {
        TRY(ln(*w.rin, n_g, n_b, w.nrm));
        ex.free(w.qkv); ex.free(w.ao); ex.free(w.hdn);
        return 0;
    }
    // bu = lrelu_0.01(conv_before_upsample(*w.u)) at 64 channels; every trunk tensor is released
    int before_upsample(Bufs& w, Tn& bu) {
        ex.free(w.nrm); ex.free(w.feat); ex.free(*w.rin); ex.free(*w.v);
        TRY(ex.alloc(bu, w.u->B, w.u->H, w.u->W, 64));
        TRY(conv3(*w.u, conv_bu, 0, nullptr, bu));
        TRY(act(bu, 1, 0.01f));                                  // nn.LeakyReLU(inplace=True): the default slope
        ex.free(*w.u);
        return 0;
    }
    // conv_last(top) / img_range + mean -> out; top is released
    int last_and_exit(Tn& top, void* out, int odt) {
        Tn last;
        TRY(ex.alloc(last, top.B, top.H, top.W, 8));
        TRY(conv3(top, conv_last, 0, nullptr, last));
        ex.free(top);
        if (!ex.dry()) {
            if (!out) GYRE_FAIL(GYRE_ERR_INVALID, std::string(name) + ": null output buffer");
            TRY(launch_swin_exit(ex.st, last.p, last.C, last.B, (size_t)last.H * last.W, mean, img_range, out, odt));
        }
        ex.free(last);
        return 0;
    }
};
