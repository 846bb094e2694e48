// What the upscaler graphs share (model_rrdb.hip, model_swinir.hip, model_hat.hip): weight records with their registration, the
// planner convolution, and WinTrunk - everything of a window-transformer upscaler (SwinIR, HAT) that is not its attention launch, its
// extra branches or its upsampler tail.
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
#pragma once
#include "model_impl.h"

struct UpConv { bf16_t* w = nullptr; float* b = nullptr; int cin = 0, cout = 0, rows = 0; };   // cin / rows: padded input channels / weight rows
struct UpLin { bf16_t* w = nullptr; float* b = nullptr; int K = 0, N = 0; };                   // padded
// what a SwinIR block, a HAB and an OCAB each own: two norms, the position table, qkv and proj, the MLP
struct WinAttnW { float *g1, *b1, *g2, *b2, *table; UpLin qkv, proj, fc1, fc2; };
static inline int pad32(int c) { return (c + 31) / 32 * 32; }

// The planner sees every launch as if its sample ran alone - no batch-dependent split-K factor - while one of these is alive
struct BatchInvariantScope {
    const int prev = gemm_set_batch_invariant(1);
    ~BatchInvariantScope() { gemm_set_batch_invariant(prev); }
};

struct WinTrunk {
    const char* const name;        // "swinir" / "hat": the prefix of every refusal
    Store store;
    Exec ex;
    bool finalized = false;
    int C = 0, Cp = 0, heads = 0, hid = 0;
    float mean[3] = {0.4488f, 0.4371f, 0.4040f}, img_range = 1.f;
    UpConv conv_first, conv_bu, conv_last;
    float *pe_g = nullptr, *pe_b = nullptr, *n_g = nullptr, *n_b = nullptr;
    explicit WinTrunk(const char* n) : name(n) {}

    // ---- registration: every helper adds its keys in state-dict order ----
    void conv(const std::string& key, int cout, int cin, int rows, int cin_pad, UpConv& c) {
        c.cin = cin_pad; c.cout = cout; c.rows = rows;
        c.w = (bf16_t*)store.dmalloc((size_t)rows * 9 * cin_pad * 2, true);
        store.add(key + ".weight", {cout, cin, 3, 3}, PK_CONV3, c.w, rows, cin_pad);
        c.b = (float*)store.dmalloc((size_t)rows * 4, true);
        store.add(key + ".bias", {cout}, PK_VEC, c.b);
    }
    void lin(const std::string& key, int O, int I, int rows, int ipad, UpLin& l, bool conv1x1 = false) {
        l.K = ipad; l.N = rows;
        l.w = (bf16_t*)store.dmalloc((size_t)rows * ipad * 2, true);
        store.add(key + ".weight", conv1x1 ? std::vector<int64_t>{O, I, 1, 1} : std::vector<int64_t>{O, I}, PK_MAT, l.w, rows, ipad);
        l.b = (float*)store.dmalloc((size_t)rows * 4, true);
        store.add(key + ".bias", {O}, PK_VEC, l.b);
    }
    void norm(const std::string& key, float** g, float** b) {
        store.vec(key + ".weight", C, g);
        store.vec(key + ".bias", C, b);
    }
    void table(const std::string& key, int rows, WinAttnW& a) {
        a.table = (float*)store.dmalloc((size_t)rows * heads * 4, true);
        store.add(key, {rows, heads}, PK_TABLE_F32, a.table);
    }
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
        ex.store = &store;
        conv("conv_first", C, 3, Cp, 8, conv_first);
        norm("patch_embed.norm", &pe_g, &pe_b);
        return 0;
    }
    int check_allocs() const {
        for (void* a : store.allocs) if (!a) GYRE_FAIL(GYRE_ERR_HIP, "hipMalloc failed");
        return 0;
    }

    // ---- execution ----
    // a dry run plans with aligned stand-ins (arena tensors are 256-byte aligned)
    bf16_t* at(const Tn& t) const { return ex.arena.dry ? (bf16_t*)(uintptr_t)4096 : t.p; }
    // out = conv3x3(x) + bias (+ res); ups: nearest 2x inside the gather.  The plain planner convolution: the caller owns `out`, no
    // column statistics, no four-parity form
    int conv3(const Tn& x, const UpConv& c, int ups, const Tn* res, Tn& out) {
        const int Ho = ups ? 2 * x.H : x.H, Wo = ups ? 2 * x.W : x.W;
        if (x.C != c.cin || out.C != c.rows || out.H != Ho || out.W != Wo || out.B != x.B || (res && res->C != out.C))
            GYRE_FAIL(GYRE_ERR_INVALID, std::string(name) + ": internal shape mismatch");
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
    int linear(const Tn& x, const UpLin& l, const Tn* res, Tn& out) {
        if (x.C != l.K || out.C != l.N || (res && res->C != l.N)) GYRE_FAIL(GYRE_ERR_INVALID, std::string(name) + ": internal shape mismatch");
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
        ex.arena.reset((char*)ws, wsb, dry); ex.st = st; ex.batch = B; ex.cs_unit = 0;
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
