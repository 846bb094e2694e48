// ControlNet forward graph (hint image + latents + timestep + text context -> one residual per UNet skip connection and one for the
// mid block) and its C ABI (include/gyre_hip.h).
//
// Topology restates the control model the reference vendors
//   gyre/pipeline/controlnet/models.py:41-94     the conditioning embedding of the hint image (eight 3x3 convolutions, SiLU between)
//   gyre/pipeline/controlnet/models.py:153-282   a copy of the UNet's conv_in / time embedding / down blocks / mid block, plus one
//                                                1x1 "zero convolution" per skip connection and one for the mid block
//   gyre/pipeline/controlnet/models.py:488-544   forward: conv_in(latents) + embedding, down path, mid block, zero convolutions, scales
// driven once per denoising step from gyre/pipeline/unet/core.py:40-64; weights are addressed by the diffusers ControlNetModel
// state-dict keys.  The copied half is the UNet's own: both handles are a UNetTrunk (model_impl.h) - one config check, one registration of
// time embedding / conv_in / down levels / mid block (the conditioning embedding registers through its hook, between conv_in and
// down_blocks.0), one project_context, one time_embed prologue.  The walk stays this file's: it emits a zero convolution after
// every step and has no up path, conv_out, ToMe or input gradients.  What does not depend on the step - the embedding of the hint
// image and the cross-attention K / V of the text context - is computed once per request (bind) and kept in buffers the handle owns.
#include "model_impl.h"

struct gyre_ctrl : UNetTrunk {        // the trunk, then the embedding of the hint image and the zero convolutions
    gyre_ctrl_cfg cfg;
    Store store;
    Exec ex;
    bool finalized = false;
    ConvW ce_in, ce_out;                      // controlnet_cond_embedding.conv_in / .conv_out
    std::vector<ConvW> ce_blocks;             // .blocks.0 .. : (stride 1, stride 2) pairs
    std::vector<ConvW> zero;                  // controlnet_down_blocks.k, one per skip connection (1x1)
    ConvW zero_mid;                           // controlnet_mid_block (1x1)
    // per-request state (bind), GYRE_CTRL_SLOTS independent entries - the leaves of a hires-fix / graft tree alternate on one control
    // model every step, each with its own hint image and context: the embedded hint image [B][H/8][W/8][C0], the projected text context
    // and, for a masked hint, one fp32 mask [mask_B][h_k][w_k] per residual (mask_off[k]: its first float in mask_buf)
    struct Slot {
        void* emb_buf = nullptr; size_t emb_bytes = 0;
        int emb_B = 0, emb_H = 0, emb_W = 0;
        std::vector<CtxKV> kv; void* kv_buf = nullptr; size_t kv_bytes = 0; int ctx_S = 0;
        float* mask_buf = nullptr; size_t mask_bytes = 0; std::vector<size_t> mask_off; int mask_B = 0;
        bool bound = false;
    };
    Slot slots[GYRE_CTRL_SLOTS];
    std::vector<CtxKV> dry_kv;                // what a sizing walk counts its cached layers in
    void drop_slots() { for (auto& sl : slots) sl.bound = false; }
    std::map<std::array<long, 5>, size_t> ws_memo;   // gyre_ctrl_workspace_bytes is asked before every step: peak per (B, H, W, S, planner state)
    ~gyre_ctrl() {
        for (auto& sl : slots) {
            if (sl.emb_buf) (void)hipFree(sl.emb_buf);
            if (sl.kv_buf) (void)hipFree(sl.kv_buf);
            if (sl.mask_buf) (void)hipFree(sl.mask_buf);
        }
    }

    int n_outputs() const { return (int)zero.size() + 1; }
    void reg3(const std::string& key, int cout, int cin, ConvW& c) { c.cin = pad8(cin); c.cout = cout; c.w = store.conv3(key, cout, cin, &c.b); }
    void reg1(const std::string& key, int cout, int cin, ConvW& c) { c.cin = cin; c.cout = cout; c.w = store.mat(key, cout, cin, true, true, &c.b); }

    int build() {
        const gyre_ctrl_cfg& c = cfg;
        const int n = c.n_levels;
        // this model's own checks come before the shared ones (UNetTrunk::check_cfg divides by num_heads)
        if (n < 1 || n > GYRE_MAX_LEVELS) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: n_levels out of range");
        if (c.in_channels < 1 || c.cond_channels < 1 || c.layers_per_block < 1) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: bad channel / layer count");
        for (int i = 0; i < n; ++i) {
            if (c.block_out_channels[i] < 8) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: block_out_channels must be multiples of norm_num_groups and 8");
            if (c.attn_levels[i] && c.num_heads[i] < 1) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: head dim must be a multiple of 8");
        }
        TRY(check_cfg(c, "ctrl: "));
        for (int i = 0; i < 4; ++i)
            if (c.cond_embed_channels[i] < 8 || c.cond_embed_channels[i] % 8)
                GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: conditioning embedding widths must be positive multiples of 8");
        const int c0 = c.block_out_channels[0];
        TRY(build_trunk(store, ex, c, 0, [&] {
            // the embedding of the hint image: conv_in, (stride 1, stride 2) per width change, conv_out up to the UNet's first width
            reg3("controlnet_cond_embedding.conv_in", c.cond_embed_channels[0], c.cond_channels, ce_in);
            for (int i = 0; i < 3; ++i) {
                const int ci = c.cond_embed_channels[i], co = c.cond_embed_channels[i + 1];
                ce_blocks.emplace_back(); reg3("controlnet_cond_embedding.blocks." + std::to_string(2 * i), ci, ci, ce_blocks.back());
                ce_blocks.emplace_back(); reg3("controlnet_cond_embedding.blocks." + std::to_string(2 * i + 1), co, ci, ce_blocks.back());
            }
            reg3("controlnet_cond_embedding.conv_out", c0, c.cond_embed_channels[3], ce_out);
        }));
        zero.resize(skip_ch.size());
        for (size_t k = 0; k < skip_ch.size(); ++k) reg1("controlnet_down_blocks." + std::to_string(k), skip_ch[k], skip_ch[k], zero[k]);
        reg1("controlnet_mid_block", skip_ch.back(), skip_ch.back(), zero_mid);
        return build_done(store);
    }

    // ---- once per request ----------------------------------------------------------------------------------------------------
    int silu(Tn& t) { return ex.dry() ? 0 : launch_silu(ex.st, t.p, (size_t)t.rows() * t.C); }
    // The hint image [Bi][cond_channels][H][W] (Bi == B, or 1: the one image serves every sample) -> emb_buf [B][H/8][W/8][C0].
    // A single image is repeated along the batch BEFORE the convolutions: a launch over B samples may plan its tiles and K splits
    // differently from one over a single sample, and a request must not change its bits with the way the caller batched the hint.
    int run_bind(bool dry, hipStream_t st, Slot* sl, const void* img, int idt, int Bi, int H, int W, int B, void* ws, size_t wsb) {
        const gyre_ctrl_cfg& c = cfg;
        if (B < 1 || (Bi != B && Bi != 1)) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: the hint image needs batch 1 or the batch of the latents");
        if (H < 8 || W < 8 || (H & 7) || (W & 7)) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: hint image height and width must be positive multiples of 8");
        ex.arena.reset((char*)ws, wsb, dry); ex.st = st; ex.batch = B; ex.cs_unit = 0;
        ex.ctx_cache = nullptr; ex.ctx_layer = 0;
        Tn x, y;
        TRY(ex.alloc(x, B, H, W, pad8(c.cond_channels)));
        if (!dry) {
            TRY(launch_nchw_to_nhwc(st, img, idt, Bi, c.cond_channels, H * W, x.C, x.p));
            const size_t one = (size_t)H * W * x.C * 2;
            for (int b = Bi; b < B; ++b) GYRE_HIP_CHECK(hipMemcpyAsync((char*)x.p + b * one, x.p, one, hipMemcpyDeviceToDevice, st));
        }
        TRY(ex.conv3(x, ce_in, 1, 1, 0, nullptr, 0, nullptr, y));
        ex.free(x); x = y;
        TRY(silu(x));
        for (size_t k = 0; k < ce_blocks.size(); ++k) {
            TRY(ex.conv3(x, ce_blocks[k], (k & 1) ? 2 : 1, 1, 0, nullptr, 0, nullptr, y));
            ex.free(x); x = y;
            TRY(silu(x));
        }
        TRY(ex.conv3(x, ce_out, 1, 1, 0, nullptr, 0, nullptr, y));
        ex.free(x);
        if (y.H != H / 8 || y.W != W / 8) GYRE_FAIL(GYRE_ERR_INVALID, "internal: embedding size mismatch");
        if (!dry) {
            if (y.bytes > sl->emb_bytes) {
                if (sl->emb_buf) { GYRE_HIP_CHECK(hipStreamSynchronize(st)); (void)hipFree(sl->emb_buf); sl->emb_buf = nullptr; sl->emb_bytes = 0; }
                GYRE_HIP_CHECK(hipMalloc(&sl->emb_buf, y.bytes));
                sl->emb_bytes = y.bytes;
            }
            GYRE_HIP_CHECK(hipMemcpyAsync(sl->emb_buf, y.p, y.bytes, hipMemcpyDeviceToDevice, st));
            sl->emb_B = B; sl->emb_H = y.H; sl->emb_W = y.W;
        }
        ex.free(y);
        return 0;
    }

    // ---- once per step ---------------------------------------------------------------------------------------------------------
    // zero convolution of one collected tensor (bias in the epilogue), then the scaled hand-off to the caller's NCHW buffer
    int emit(const Tn& s, const ConvW& z, float scale, int accumulate, void* out, int odt, int out_B, int out_b0, const float* mask,
             int mask_B) {
        Tn r;
        TRY(ex.alloc(r, s.B, s.H, s.W, pad8(z.cout)));
        TRY(ex.linear(s.p, s.C, nullptr, 0, 0, s.rows(), s.C, z.w, r.C, z.b, nullptr, 0, 0, r.p, r.C));
        if (!ex.dry()) {
            if (!out) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: null residual buffer");
            TRY(launch_ctrl_emit_masked(ex.st, r.p, r.B, z.cout, r.H * r.W, r.C, scale, accumulate, out, odt, out_B, out_b0, mask, mask_B));
        }
        ex.free(r);
        return 0;
    }
    // The (h, w) of the N + 1 residuals for H x W latents, in emit order (a stride-2 convolution rounds an odd size up).
    std::vector<std::array<int, 2>> residual_hw(int H, int W) const {
        std::vector<std::array<int, 2>> out{{H, W}};
        int h = H, w = W;
        for (int i = 0; i < cfg.n_levels; ++i) {
            for (int j = 0; j < cfg.layers_per_block; ++j) out.push_back({h, w});
            if (i < cfg.n_levels - 1) { h = (h + 1) / 2; w = (w + 1) / 2; out.push_back({h, w}); }
        }
        out.push_back({h, w});
        return out;
    }
    // sl == nullptr: a sizing walk (dry)
    int run(bool dry, hipStream_t st, Slot* sl, const void* x, int xdt, const int64_t* t, int B, int H, int W, int S, void* ws, size_t wsb,
            const float* scales, int accumulate, int out_B, int out_b0, void* const* outs, int odt, const float* x_mask = nullptr,
            int x_mask_B = 0) {
        const gyre_ctrl_cfg& c = cfg;
        const int n = c.n_levels, D = c.cross_attention_dim;
        if (B < 1 || H < 1 || W < 1 || S < 1) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: empty batch / image / context");
        ex.arena.reset((char*)ws, wsb, dry);
        ex.st = st; ex.batch = B; ex.cs_unit = gn_unit; ex.keep_proj_out = false;
        if (dry) {                                   // sizing: the walk only counts the cached layers
            size_t layers = 0;
            for_each_cross_attn([&](AttnW&) { ++layers; });
            if (dry_kv.size() < layers) dry_kv.resize(layers, CtxKV{nullptr, nullptr});
        }
        ex.ctx_cache = dry ? &dry_kv : &sl->kv; ex.ctx_layer = 0;
        Exec& e = ex;
        Tn xin, cx, tp, bound_emb;
        xin_mask = dry ? nullptr : x_mask; xin_mask_B = x_mask_B;
        const int te = time_embed(e, c, x, xdt, B, H, W, nullptr, 0, 0, t, B, B, nullptr, xin, cx, tp);
        xin_mask = nullptr; xin_mask_B = 0;
        TRY(te);
        const float* tproj = (const float*)tp.p;
        const bool masked = !dry && !sl->mask_off.empty();
        auto mask_k = [&](int i) -> const float* { return masked ? sl->mask_buf + sl->mask_off[i] : nullptr; };
        const int mB = masked ? sl->mask_B : 0;
        // conv_in(latents) + embedded hint: the embedding rides as the convolution's residual
        bound_emb.p = dry ? nullptr : (bf16_t*)sl->emb_buf; bound_emb.B = B; bound_emb.H = H; bound_emb.W = W; bound_emb.C = pad8(c.block_out_channels[0]);
        Tn h;
        TRY(e.conv3(xin, conv_in, 1, 1, 0, nullptr, 0, &bound_emb, h));
        e.free(xin);
        int k = 0;
        auto out_k = [&](int i) -> void* { return dry ? nullptr : outs[i]; };
        TRY(emit(h, zero[k], dry ? 0.f : scales[k], accumulate, out_k(k), odt, out_B, out_b0, mask_k(k), mB)); ++k;
        for (int i = 0; i < n; ++i) {
            for (int j = 0; j < c.layers_per_block; ++j) {
                Tn r;
                TRY(e.resnet(h, nullptr, down[i].res[j], tproj, temb_cols, 1e-5f, r));
                e.free(h);
                if (c.attn_levels[i]) {
                    Tn a;
                    TRY(e.transformer(r, cx, S, D, down[i].attn[j], a));
                    e.free(r); r = a;
                }
                h = r;
                TRY(emit(h, zero[k], dry ? 0.f : scales[k], accumulate, out_k(k), odt, out_B, out_b0, mask_k(k), mB)); ++k;
            }
            if (down[i].has_resample) {
                Tn d;
                TRY(e.conv3(h, down[i].resample, 2, 1, 0, nullptr, 0, nullptr, d));
                e.free(h); h = d;
                TRY(emit(h, zero[k], dry ? 0.f : scales[k], accumulate, out_k(k), odt, out_B, out_b0, mask_k(k), mB)); ++k;
            }
        }
        {
            Tn a, b2, m;
            TRY(e.resnet(h, nullptr, mid0, tproj, temb_cols, 1e-5f, a));
            e.free(h);
            TRY(e.transformer(a, cx, S, D, mid_attn, b2));
            e.free(a);
            TRY(e.resnet(b2, nullptr, mid1, tproj, temb_cols, 1e-5f, m));
            e.free(b2);
            TRY(emit(m, zero_mid, dry ? 0.f : scales[k], accumulate, out_k(k), odt, out_B, out_b0, mask_k(k), mB));
            e.free(m);
        }
        e.free(tp);
        return 0;
    }
    // the peak over the forms a forward of this shape can take: proj_out folded into FF2 or not (Exec::proj_out_folds)
    size_t forward_workspace(int B, int H, int W, int S) {
        const std::array<long, 5> key{B, H, W, S, gemm_planner_state()};
        auto it = ws_memo.find(key);
        if (it != ws_memo.end()) return it->second;
        size_t peak = 0;
        for (int fold = 0; fold <= 1; ++fold) {
            ex.pout_fold_dry = fold;
            const int rc = run(true, nullptr, nullptr, nullptr, 0, nullptr, B, H, W, S, nullptr, 0, nullptr, 0, B, 0, nullptr, 0);
            ex.pout_fold_dry = -1;
            if (rc) return 0;
            peak = std::max(peak, ex.arena.peak);
        }
        if (ws_memo.size() > 64) ws_memo.clear();
        ws_memo[key] = peak;
        return peak;
    }
};

extern "C" {

int gyre_ctrl_create(const gyre_ctrl_cfg* cfg, int device, gyre_ctrl** out) { return handle_create(cfg, device, out); }
void gyre_ctrl_destroy(gyre_ctrl* h) { delete h; }
int gyre_ctrl_num_params(const gyre_ctrl* h) { return handle_num_params(h); }
const char* gyre_ctrl_param_key(const gyre_ctrl* h, int i) { return handle_param_key(h, i); }
int gyre_ctrl_set_weight(gyre_ctrl* h, const char* key, const void* p, int dtype, const int64_t* shape, int ndim, void* st) {
    if (!h || !key || !p || !shape) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    h->finalized = false;
    h->drop_slots();                             // the embeddings and the projected contexts were made with the old weights
    return h->store.set_weight(key, p, dtype, shape, ndim, (hipStream_t)st);
}
int gyre_ctrl_finalize(gyre_ctrl* h, void* st) { return handle_finalize(h); }
size_t gyre_ctrl_bind_workspace_bytes(gyre_ctrl* h, int image_B, int image_H, int image_W, int B) {
    if (!h) return 0;
    return h->run_bind(true, nullptr, nullptr, nullptr, 0, image_B, image_H, image_W, B, nullptr, 0) ? 0 : h->ex.arena.peak;
}
size_t gyre_ctrl_bind_slot_workspace_bytes(gyre_ctrl* h, int slot, int image_B, int image_H, int image_W, int B) {
    if (!h) return 0;
    if (slot < 0 || slot >= GYRE_CTRL_SLOTS) { gyre_set_error("ctrl: bind slot out of range"); return 0; }
    return gyre_ctrl_bind_workspace_bytes(h, image_B, image_H, image_W, B);      // (the masks live in buffers the handle owns)
}
int gyre_ctrl_bind_slot(gyre_ctrl* h, void* st, int slot, const void* image, int idt, int image_B, int image_H, int image_W,
                        const void* ctx, int cdt, int B, int S, const float* const* res_masks, const int32_t* mask_hw, int n_masks,
                        int mask_B, void* ws, size_t wsb) {
    if (!h || !image || !ctx || !ws) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    if (slot < 0 || slot >= GYRE_CTRL_SLOTS) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: bind slot out of range");
    if (!h->finalized) GYRE_FAIL(GYRE_ERR_INCOMPLETE, "gyre_ctrl_finalize has not succeeded");
    if (idt < 0 || idt > 2 || cdt < 0 || cdt > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    if (B < 1 || S < 1) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: empty context");
    gyre_ctrl::Slot& sl = h->slots[slot];
    // the residual masks: none of them, or one per residual at exactly that residual's size
    bool masked = false;
    if (res_masks)
        for (int i = 0; i < n_masks; ++i) masked = masked || res_masks[i];
    std::vector<size_t> off;
    size_t floats = 0;
    if (masked) {
        if (n_masks != h->n_outputs() || !mask_hw)
            GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: " + std::to_string(h->n_outputs()) + " residual masks (and their sizes) expected, or none");
        if (mask_B != 1 && mask_B != B) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: the residual masks need batch 1 or the batch of the latents");
        if (image_H < 8 || image_W < 8 || (image_H & 7) || (image_W & 7))
            GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: hint image height and width must be positive multiples of 8");
        const auto hw = h->residual_hw(image_H / 8, image_W / 8);
        for (int i = 0; i < n_masks; ++i) {
            if (!res_masks[i]) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: residual mask " + std::to_string(i) + " is null while others are set");
            if (mask_hw[2 * i] != hw[i][0] || mask_hw[2 * i + 1] != hw[i][1])
                GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: residual mask " + std::to_string(i) + " is " + std::to_string(mask_hw[2 * i]) + " x " +
                          std::to_string(mask_hw[2 * i + 1]) + ", the residual " + std::to_string(hw[i][0]) + " x " + std::to_string(hw[i][1]));
            off.push_back(floats);
            floats += align_up((size_t)mask_B * hw[i][0] * hw[i][1], 64);
        }
    }
    gyre_launch_counter() = 0;
    sl.bound = false;
    TRY(h->run_bind(false, (hipStream_t)st, &sl, image, idt, image_B, image_H, image_W, B, ws, wsb));
    // the cross-attention K / V^T of the text context through this model's own to_k / to_v, as gyre_unet::set_context keeps the UNet's
    TRY(project_context((hipStream_t)st, ctx, cdt, B, S, h->cfg.cross_attention_dim, [&](auto f) { h->for_each_cross_attn(f); }, sl.kv_buf,
                        sl.kv_bytes, sl.kv));
    sl.ctx_S = S;
    sl.mask_off.clear(); sl.mask_B = 0;
    if (masked) {
        if (floats * 4 > sl.mask_bytes) {
            if (sl.mask_buf) { GYRE_HIP_CHECK(hipStreamSynchronize((hipStream_t)st)); (void)hipFree(sl.mask_buf); sl.mask_buf = nullptr; sl.mask_bytes = 0; }
            GYRE_HIP_CHECK(hipMalloc((void**)&sl.mask_buf, floats * 4));
            sl.mask_bytes = floats * 4;
        }
        const auto hw = h->residual_hw(image_H / 8, image_W / 8);
        for (int i = 0; i < n_masks; ++i)
            GYRE_HIP_CHECK(hipMemcpyAsync(sl.mask_buf + off[i], res_masks[i], (size_t)mask_B * hw[i][0] * hw[i][1] * 4, hipMemcpyDeviceToDevice,
                                          (hipStream_t)st));
        sl.mask_off = off; sl.mask_B = mask_B;
    }
    sl.bound = true;
    return 0;
}
int gyre_ctrl_bind(gyre_ctrl* h, void* st, const void* image, int idt, int image_B, int image_H, int image_W, const void* ctx, int cdt,
                   int B, int S, void* ws, size_t wsb) {
    return gyre_ctrl_bind_slot(h, st, 0, image, idt, image_B, image_H, image_W, ctx, cdt, B, S, nullptr, nullptr, 0, 0, ws, wsb);
}
size_t gyre_ctrl_workspace_bytes(gyre_ctrl* h, int B, int H, int W, int S) {
    if (!h) return 0;
    return h->forward_workspace(B, H, W, S);
}
int gyre_ctrl_forward_slot(gyre_ctrl* h, void* st, int slot, const void* x, int xdt, const float* x_mask, int x_mask_B, const int64_t* t,
                           int B, int H, int W, void* ws, size_t wsb, const float* scales, int accumulate, int out_B, int out_b0,
                           void* const* outs, int n_outs, int odt) {
    if (!h || !x || !t || !ws || !scales || !outs) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    if (slot < 0 || slot >= GYRE_CTRL_SLOTS) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: bind slot out of range");
    if (!h->finalized) GYRE_FAIL(GYRE_ERR_INCOMPLETE, "gyre_ctrl_finalize has not succeeded");
    gyre_ctrl::Slot& sl = h->slots[slot];
    if (!sl.bound) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: forward needs a gyre_ctrl_bind call first (hint image and text context of the request)");
    if (xdt < 0 || xdt > 2 || odt < 0 || odt > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    if (B != sl.emb_B) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: the batch differs from the bound one (" + std::to_string(sl.emb_B) + ")");
    if (H != sl.emb_H || W != sl.emb_W)
        GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: latents of " + std::to_string(H) + " x " + std::to_string(W) + " do not match the bound hint image (" +
                  std::to_string(sl.emb_H) + " x " + std::to_string(sl.emb_W) + " after its 8x reduction)");
    if (x_mask && x_mask_B != 1 && x_mask_B != B) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: the latent mask needs batch 1 or the batch of the latents");
    if (n_outs != h->n_outputs()) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: " + std::to_string(h->n_outputs()) + " residual buffers expected");
    if (out_b0 < 0 || out_B < 1 || out_b0 + B > out_B) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: the samples [out_b0, out_b0 + B) must lie inside the output batch");
    for (int i = 0; i < n_outs; ++i) if (!outs[i]) GYRE_FAIL(GYRE_ERR_INVALID, "ctrl: null residual buffer");
    gyre_launch_counter() = 0;
    return h->run(false, (hipStream_t)st, &sl, x, xdt, t, B, H, W, sl.ctx_S, ws, wsb, scales, accumulate ? 1 : 0, out_B, out_b0, outs, odt,
                  x_mask, x_mask_B);
}
int gyre_ctrl_forward(gyre_ctrl* h, void* st, const void* x, int xdt, const int64_t* t, int B, int H, int W, void* ws, size_t wsb,
                      const float* scales, int accumulate, int out_B, int out_b0, void* const* outs, int n_outs, int odt) {
    return gyre_ctrl_forward_slot(h, st, 0, x, xdt, nullptr, 0, t, B, H, W, ws, wsb, scales, accumulate, out_B, out_b0, outs, n_outs, odt);
}

int gyre_op_silu(void* st, void* x, size_t n) {
    if (!x) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    return launch_silu((hipStream_t)st, (bf16_t*)x, n);
}
int gyre_op_ctrl_emit(void* st, const void* f, int B, int C, int HW, int Cpad, float scale, int accumulate, void* out, int out_dtype,
                      int out_B, int out_b0) {
    if (!f || !out) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    return launch_ctrl_emit((hipStream_t)st, (const bf16_t*)f, B, C, HW, Cpad, scale, accumulate, out, out_dtype, out_B, out_b0);
}
int gyre_op_ctrl_emit_masked(void* st, const void* f, int B, int C, int HW, int Cpad, float scale, int accumulate, void* out, int out_dtype,
                             int out_B, int out_b0, const float* mask, int mask_B) {
    if (!f || !out || !mask) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    return launch_ctrl_emit_masked((hipStream_t)st, (const bf16_t*)f, B, C, HW, Cpad, scale, accumulate, out, out_dtype, out_B, out_b0, mask,
                                   mask_B);
}
int gyre_op_nchw_to_nhwc_masked(void* st, const void* x, int dtype, int B, int C, int HW, int Cpad, const float* mask, int mask_B, void* y) {
    if (!x || !y || !mask) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    return launch_nchw_to_nhwc_masked((hipStream_t)st, x, dtype, B, C, HW, Cpad, mask, mask_B, (bf16_t*)y);
}

}  // extern "C"
