// The token-sequence T2I networks and their C ABI (include/gyre_hip.h): the style adapter and the co-adapter fuser the reference vendors
//   gyre/pipeline/t2i_adapter/adapter.py:173-199   StyleAdapter     CLIP hidden states [N][S][width] -> style tokens [N][num_token][context_dim]
//   gyre/pipeline/t2i_adapter/adapter.py:266-343   CoAdapterFuser   the states / tokens of several co-adapters -> gained states / tokens
// Both are pre-LN transformers of the CLIP kind (adapter.py:150-170 ResidualAttentionBlock) over a short sequence; weights are addressed
// by the state-dict keys of those classes.
//
//   block(x) = x + out_proj(attn(in_proj(ln_1 x)));  x + c_proj(quickgelu(c_fc(ln_2 x)))
// in_proj is ONE planner GEMM into the packed [N L][3 W] tensor k_seq_attn reads in place (kernels_seq.hip): no head split, no
// transposed V, no concatenation of heads exists as a tensor.  The sequence is sample-major (row n L + l); the reference's [L, N, E]
// is a view order only.
//
// Where values are narrowed.  The residual stream is kept in the storage type: each of the two residual additions of a block happens
// in fp32 inside the GEMM epilogue (accumulator + bias + residual) and is rounded once.  LayerNorm reads storage, computes its
// statistics and affine in fp32 and writes storage (the GEMM operand).  in_proj, c_fc (then QuickGELU in fp32, in place), the pooled
// SiLU features and the sequence rows (feature + task embedding + positional embedding, summed in fp32 in that order) are storage
// tensors.  The fuser's channel gains alpha = spatial_ch_projs[i](x) are fp32 (launch_rowvec_linear on an fp32 copy of the row); the
// token gain x @ seq_proj is a storage tensor, + 1 and the product are fp32.  A sum over co-adapters of one kind (adapter.py:337) is
// narrowed after every term, as the reference's own fp16 tensors are.
#include "model_impl.h"

struct gyre_t2i_seq {
    gyre_t2i_seq_cfg cfg;
    Store store;
    Exec ex;
    bool finalized = false;
    struct Block {
        float *ln1g = nullptr, *ln1b = nullptr, *ln2g = nullptr, *ln2b = nullptr;
        bf16_t *w_in = nullptr, *w_out = nullptr, *w_fc = nullptr, *w_proj = nullptr;
        float *b_in = nullptr, *b_out = nullptr, *b_fc = nullptr, *b_proj = nullptr;
    };
    std::vector<Block> blocks;
    float *pre_g = nullptr, *pre_b = nullptr, *post_g = nullptr, *post_b = nullptr;
    float* style_emb = nullptr; bf16_t* proj_t = nullptr;                                   // style
    float *task_emb = nullptr, *pos_emb = nullptr;                                          // fuser
    bf16_t* map_w[4] = {}; float* map_b[4] = {}; bf16_t* ch_w[4] = {}; float* ch_b[4] = {}; bf16_t* seq_proj_t = nullptr;
    int D = 0;

    bf16_t* mat_t(const std::string& key, int I, int O) {                                   // P [I][O] used as x @ P
        bf16_t* w = (bf16_t*)store.dmalloc((size_t)pad8(O) * pad8(I) * 2, true);
        store.add(key, {I, O}, PK_MAT_T, w, pad8(O), pad8(I));
        return w;
    }
    float* table(const std::string& key, std::vector<int64_t> shape) {
        size_t n = 1;
        for (auto d : shape) n *= (size_t)d;
        float* t = (float*)store.dmalloc(n * 4, true);
        store.add(key, std::move(shape), PK_TABLE_F32, t);
        return t;
    }
    int build() {
        const gyre_t2i_seq_cfg& c = cfg;
        if (c.kind != GYRE_T2I_SEQ_STYLE && c.kind != GYRE_T2I_SEQ_FUSER) GYRE_FAIL(GYRE_ERR_INVALID, "t2i_seq: kind must be 0 (style) or 1 (fuser)");
        if (c.width < 8 || c.num_head < 1 || c.n_layers < 1 || c.n_layers > 64) GYRE_FAIL(GYRE_ERR_INVALID, "t2i_seq: bad width, num_head or n_layers");
        if (c.width % c.num_head) GYRE_FAIL(GYRE_ERR_INVALID, "t2i_seq: num_head must divide width");
        D = c.width / c.num_head;
        if (!seq_attn_max_len(D)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "t2i_seq: width / num_head must be 32, 64, 96 or 128, got " + std::to_string(D));
        if (c.width > 2048) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "t2i_seq: widths up to 2048 (LayerNorm kernel)");
        const int W = c.width;
        ex.store = &store;
        if (c.kind == GYRE_T2I_SEQ_STYLE) {
            if (c.num_token < 1 || c.context_dim < 1) GYRE_FAIL(GYRE_ERR_INVALID, "t2i_seq: num_token and context_dim must be positive");
            style_emb = table("style_embedding", {1, c.num_token, W});
            proj_t = mat_t("proj", W, c.context_dim);
        } else {
            for (int i = 0; i < 4; ++i)
                if (c.unet_channels[i] < 8 || c.unet_channels[i] % 8)
                    GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "t2i_seq: the fuser's channel counts must be positive multiples of 8");
            task_emb = table("task_embedding", {16, W});
            pos_emb = table("positional_embedding", {4, W});
            for (int i = 0; i < 4; ++i) {
                map_w[i] = store.mat("spatial_feat_mapping." + std::to_string(i) + ".1", W, c.unet_channels[i], false, true, &map_b[i]);
                ch_w[i] = store.mat("spatial_ch_projs." + std::to_string(i), c.unet_channels[i], W, false, true, &ch_b[i]);
            }
            seq_proj_t = mat_t("seq_proj", W, W);
        }
        for (int l = 0; l < c.n_layers; ++l) {
            const std::string p = "transformer_layes." + std::to_string(l);
            Block b;
            b.w_in = (bf16_t*)store.dmalloc((size_t)3 * W * W * 2, true);
            store.add(p + ".attn.in_proj_weight", {3 * W, W}, PK_MAT, b.w_in, 3 * W, W);
            store.vec(p + ".attn.in_proj_bias", 3 * W, &b.b_in);
            b.w_out = store.mat(p + ".attn.out_proj", W, W, false, true, &b.b_out);
            store.vec(p + ".ln_1.weight", W, &b.ln1g); store.vec(p + ".ln_1.bias", W, &b.ln1b);
            b.w_fc = store.mat(p + ".mlp.c_fc", 4 * W, W, false, true, &b.b_fc);
            b.w_proj = store.mat(p + ".mlp.c_proj", W, 4 * W, false, true, &b.b_proj);
            store.vec(p + ".ln_2.weight", W, &b.ln2g); store.vec(p + ".ln_2.bias", W, &b.ln2b);
            blocks.push_back(b);
        }
        store.vec("ln_post.weight", W, &post_g); store.vec("ln_post.bias", W, &post_b);
        store.vec("ln_pre.weight", W, &pre_g); store.vec("ln_pre.bias", W, &pre_b);
        for (void* a : store.allocs) if (!a) GYRE_FAIL(GYRE_ERR_HIP, "hipMalloc failed");
        return 0;
    }

    int lin(const Tn& x, const bf16_t* w, int Nout, const float* bias, const Tn* residual, Tn& y) {
        TRY(ex.alloc(y, x.B, x.H, x.W, Nout));
        return ex.linear(x.p, x.C, nullptr, 0, 0, x.rows(), x.C, w, Nout, bias, residual ? residual->p : nullptr, residual ? residual->C : 0, 0,
                         y.p, Nout);
    }
    // x [N][1][L][W] -> the block's output in x
    int block(Tn& x, const Block& b) {
        const int W = cfg.width, N = x.B, L = x.W;
        Tn h, qkv, a, y;
        TRY(ex.layernorm(x, b.ln1g, b.ln1b, h));
        TRY(lin(h, b.w_in, 3 * W, b.b_in, nullptr, qkv));
        ex.free(h);
        TRY(ex.alloc(a, N, 1, L, W));
        if (!ex.dry()) TRY(launch_seq_attn(ex.st, qkv.p, 3 * W, a.p, W, N, L, cfg.num_head, D));
        ex.free(qkv);
        TRY(lin(a, b.w_out, W, b.b_out, &x, y));
        ex.free(a); ex.free(x); x = y;
        TRY(ex.layernorm(x, b.ln2g, b.ln2b, h));
        TRY(lin(h, b.w_fc, 4 * W, b.b_fc, nullptr, a));
        ex.free(h);
        if (!ex.dry()) TRY(launch_quick_gelu(ex.st, a.p, (size_t)a.rows() * a.C));
        TRY(lin(a, b.w_proj, W, b.b_proj, &x, y));
        ex.free(a); ex.free(x); x = y;
        return 0;
    }
    // ln_pre, then the blocks, on the assembled sequence
    int trunk(Tn& x) {
        Tn h;
        TRY(ex.layernorm(x, pre_g, pre_b, h));
        ex.free(x); x = h;
        for (const Block& b : blocks) TRY(block(x, b));
        return 0;
    }
    int begin(bool dry, hipStream_t st, int N, int L, void* ws, size_t wsb) {
        if (N < 1 || L < 1) GYRE_FAIL(GYRE_ERR_INVALID, "t2i_seq: the batch and the sequence must not be empty");
        if (L > seq_attn_max_len(D))
            GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "t2i_seq: a sequence of " + std::to_string(L) + " tokens exceeds the " + std::to_string(seq_attn_max_len(D)) +
                                                " the attention kernel holds at head dim " + std::to_string(D));
        if ((size_t)N * L * 4 * cfg.width >= (1ull << 31)) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "t2i_seq: the batch is too large");
        ex.arena.reset((char*)ws, wsb, dry); ex.st = st; ex.batch = N; ex.cs_unit = 0;
        return 0;
    }

    int run_style(bool dry, hipStream_t st, const void* xin, int xdt, int N, int S, void* ws, size_t wsb, void* out, int odt) {
        const gyre_t2i_seq_cfg& c = cfg;
        if (c.kind != GYRE_T2I_SEQ_STYLE) GYRE_FAIL(GYRE_ERR_INVALID, "t2i_seq: not a style adapter");
        if (S < 1) GYRE_FAIL(GYRE_ERR_INVALID, "t2i_seq: the input sequence must not be empty");
        const int W = c.width, T = c.num_token, L = S + T, Cp = pad8(c.context_dim);
        TRY(begin(dry, st, N, L, ws, wsb));
        Tn x, y, o;
        TRY(ex.alloc(x, N, 1, L, W));
        if (!dry) {
            SeqRows a;                                                  // cat[x, style_embedding] (adapter.py:188-190)
            a.src = xin; a.src_dtype = xdt; a.src_ss = (size_t)S * W; a.src_rs = W;
            a.dst = x.p; a.dst_dtype = GYRE_STORAGE_DTYPE; a.dst_ss = (size_t)L * W; a.dst_rs = W; a.N = N; a.R = S; a.W = W;
            TRY(launch_seq_rows(st, a));
            a.src = nullptr; a.add1 = style_emb; a.dst = x.p + (size_t)S * W; a.R = T;
            TRY(launch_seq_rows(st, a));
        }
        TRY(trunk(x));
        Tn last;                                                        // the last num_token rows of every sample, gathered (bit copies) ...
        TRY(ex.alloc(last, N, 1, T, W));
        if (!dry) {
            SeqRows a;
            a.src = x.p + (size_t)S * W; a.src_dtype = GYRE_STORAGE_DTYPE; a.src_ss = (size_t)L * W; a.src_rs = W;
            a.dst = last.p; a.dst_dtype = GYRE_STORAGE_DTYPE; a.dst_ss = (size_t)T * W; a.dst_rs = W; a.N = N; a.R = T; a.W = W;
            TRY(launch_seq_rows(st, a));
        }
        ex.free(x);
        TRY(ex.layernorm(last, post_g, post_b, y));                     // ... and ln_post over them in one launch
        ex.free(last);
        TRY(lin(y, proj_t, Cp, nullptr, nullptr, o));
        ex.free(y);
        if (!dry) TRY(launch_nhwc_to_nchw(st, o.p, N * T, c.context_dim, 1, Cp, out, odt));
        ex.free(o);
        return 0;
    }

    int run_fuser(bool dry, hipStream_t st, const gyre_fuser_input* in, int n_in, int tdt, int N, void* ws, size_t wsb, void* const* maps_out,
                  void* tokens_out) {
        const gyre_t2i_seq_cfg& c = cfg;
        if (c.kind != GYRE_T2I_SEQ_FUSER) GYRE_FAIL(GYRE_ERR_INVALID, "t2i_seq: not a fuser");
        if (!in || n_in < 1 || n_in > 16) GYRE_FAIL(GYRE_ERR_INVALID, "t2i_seq: 1 to 16 fuser inputs");
        const int W = c.width;
        int L = 0, Ttot = 0, n_sp = 0, hw[4] = {0, 0, 0, 0};
        for (int e = 0; e < n_in; ++e) {
            if (in[e].task < 0 || in[e].task > 15) GYRE_FAIL(GYRE_ERR_INVALID, "t2i_seq: the task index is 0 .. 15");
            if (in[e].tokens < 0 || in[e].tokens > 4096) GYRE_FAIL(GYRE_ERR_INVALID, "t2i_seq: bad token count");
            if (in[e].tokens) { L += in[e].tokens; Ttot += in[e].tokens; continue; }
            for (int i = 0; i < 4; ++i) {
                if (in[e].h[i] < 1 || in[e].w[i] < 1) GYRE_FAIL(GYRE_ERR_INVALID, "t2i_seq: empty feature map");
                if (n_sp && in[e].h[i] * in[e].w[i] != hw[i]) GYRE_FAIL(GYRE_ERR_INVALID, "t2i_seq: the co-adapters' states differ in size");
                hw[i] = in[e].h[i] * in[e].w[i];
            }
            L += 4; ++n_sp;
        }
        if (!dry) {
            if ((n_sp && !maps_out) || (Ttot && !tokens_out)) GYRE_FAIL(GYRE_ERR_INVALID, "t2i_seq: null output");
            for (int e = 0; e < n_in; ++e)
                for (int i = 0; i < (in[e].tokens ? 1 : 4); ++i)
                    if (!in[e].in[i] || (!in[e].tokens && !maps_out[i])) GYRE_FAIL(GYRE_ERR_INVALID, "t2i_seq: null input or output");
        }
        TRY(begin(dry, st, N, L, ws, wsb));
        Tn x, y, g;
        TRY(ex.alloc(x, N, 1, L, W));
        int off = 0;
        for (int e = 0; e < n_in; ++e) {                                // the sequence, in the caller's order (adapter.py:291-307)
            SeqRows a;
            a.add0 = task_emb + (size_t)in[e].task * W;
            a.dst = dry ? nullptr : x.p + (size_t)off * W; a.dst_dtype = GYRE_STORAGE_DTYPE; a.dst_ss = (size_t)L * W; a.dst_rs = W; a.N = N; a.W = W;
            if (in[e].tokens) {
                a.src = in[e].in[0]; a.src_dtype = tdt; a.src_ss = (size_t)in[e].tokens * W; a.src_rs = W; a.R = in[e].tokens;
                if (!dry) TRY(launch_seq_rows(st, a));
                off += in[e].tokens;
                continue;
            }
            Tn f;
            TRY(ex.alloc(f, N, 1, 4, W));
            for (int i = 0; i < 4; ++i) {
                const int Ci = c.unet_channels[i];
                Tn p;
                TRY(ex.alloc(p, N, 1, 1, Ci));
                if (!dry) TRY(launch_fuser_pool(st, (const bf16_t*)in[e].in[i], N, Ci, (size_t)hw[i], p.p, Ci));
                TRY(ex.linear(p.p, Ci, nullptr, 0, 0, N, Ci, map_w[i], W, map_b[i], nullptr, 0, 0, dry ? nullptr : f.p + (size_t)i * W, 4 * W));
                ex.free(p);
            }
            a.src = f.p; a.src_dtype = GYRE_STORAGE_DTYPE; a.src_ss = (size_t)4 * W; a.src_rs = W; a.add1 = pos_emb; a.R = 4;
            if (!dry) TRY(launch_seq_rows(st, a));
            ex.free(f);
            off += 4;
        }
        TRY(trunk(x));
        TRY(ex.layernorm(x, post_g, post_b, y));
        ex.free(x);
        if (Ttot) TRY(lin(y, seq_proj_t, W, nullptr, nullptr, g));      // x @ seq_proj over every row; the token rows are read below
        const size_t esz = tdt == 0 ? 4 : 2;
        off = 0;
        int tok_off = 0;
        bool first = true;
        for (int e = 0; e < n_in; ++e) {                                // adapter.py:317-338
            if (in[e].tokens) {
                if (!dry) {
                    SeqTokenGain a;
                    a.tok = in[e].in[0]; a.g = g.p + (size_t)off * W; a.g_ss = (size_t)L * W; a.dtype = tdt;
                    a.out = (char*)tokens_out + (size_t)tok_off * W * esz; a.out_ss = (size_t)Ttot * W; a.N = N; a.T = in[e].tokens; a.W = W;
                    TRY(launch_seq_token_gain(st, a));
                }
                off += in[e].tokens; tok_off += in[e].tokens;
                continue;
            }
            for (int i = 0; i < 4; ++i) {
                const int Ci = c.unet_channels[i];
                Tn row, al;
                TRY(ex.alloc_raw(row, (size_t)N * W * 4));
                TRY(ex.alloc_raw(al, (size_t)N * Ci * 4));
                if (!dry) {
                    SeqRows a;                                          // row off + i of every sample, as fp32
                    a.src = y.p + (size_t)(off + i) * W; a.src_dtype = GYRE_STORAGE_DTYPE; a.src_ss = (size_t)L * W;
                    a.dst = row.p; a.dst_dtype = 0; a.dst_ss = W; a.N = N; a.R = 1; a.W = W;
                    TRY(launch_seq_rows(st, a));
                    TRY(launch_rowvec_linear(st, (float*)row.p, N, W, ch_w[i], ch_b[i], Ci, 0, (float*)al.p, Ci));
                    TRY(launch_fuser_gain(st, (const bf16_t*)in[e].in[i], (const float*)al.p, Ci, N, Ci, (size_t)hw[i], (bf16_t*)maps_out[i], first ? 0 : 1));
                }
                ex.free(row); ex.free(al);
            }
            first = false;
            off += 4;
        }
        if (Ttot) ex.free(g);
        ex.free(y);
        return 0;
    }
};

extern "C" {

int gyre_t2i_seq_create(const gyre_t2i_seq_cfg* cfg, int device, gyre_t2i_seq** out) { return handle_create(cfg, device, out); }
void gyre_t2i_seq_destroy(gyre_t2i_seq* h) { delete h; }
int gyre_t2i_seq_num_params(const gyre_t2i_seq* h) { return handle_num_params(h); }
const char* gyre_t2i_seq_param_key(const gyre_t2i_seq* h, int i) { return handle_param_key(h, i); }
int gyre_t2i_seq_set_weight(gyre_t2i_seq* h, const char* key, const void* p, int dtype, const int64_t* shape, int ndim, void* st) {
    return handle_set_weight(h, key, p, dtype, shape, ndim, st);
}
int gyre_t2i_seq_finalize(gyre_t2i_seq* h, void* st) { return handle_finalize(h); }
size_t gyre_t2i_seq_workspace_bytes(gyre_t2i_seq* h, int N, int S, int n_spatial) {
    if (!h) return 0;
    if (h->cfg.kind == GYRE_T2I_SEQ_STYLE) return h->run_style(true, nullptr, nullptr, 0, N, S, nullptr, 0, nullptr, 0) ? 0 : h->ex.arena.peak;
    if (n_spatial < 0 || n_spatial > 15 || S < 0) { gyre_set_error("t2i_seq: bad sizes"); return 0; }
    gyre_fuser_input in[16] = {};                                       // the sizes alone decide the workspace; one pixel per map
    int n = 0;
    for (; n < n_spatial; ++n)
        for (int i = 0; i < 4; ++i) in[n].h[i] = in[n].w[i] = 1;
    if (S > 0) in[n++].tokens = S;
    return h->run_fuser(true, nullptr, in, n, 0, N, nullptr, 0, nullptr, nullptr) ? 0 : h->ex.arena.peak;
}
int gyre_t2i_style_forward(gyre_t2i_seq* h, void* st, const void* x, int in_dtype, int N, int S, void* ws, size_t wsb, void* out, int out_dtype) {
    if (!h || !x || !ws || !out) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    if (!h->finalized) GYRE_FAIL(GYRE_ERR_INCOMPLETE, "gyre_t2i_seq_finalize has not succeeded");
    if (in_dtype < 0 || in_dtype > 2 || out_dtype < 0 || out_dtype > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    gyre_launch_counter() = 0;
    return h->run_style(false, (hipStream_t)st, x, in_dtype, N, S, ws, wsb, out, out_dtype);
}
int gyre_t2i_fuser_forward(gyre_t2i_seq* h, void* st, const gyre_fuser_input* inputs, int n_inputs, int token_dtype, int N, void* ws, size_t wsb,
                           void* const* maps_out, void* tokens_out) {
    if (!h || !ws) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    if (!h->finalized) GYRE_FAIL(GYRE_ERR_INCOMPLETE, "gyre_t2i_seq_finalize has not succeeded");
    if (token_dtype < 0 || token_dtype > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    gyre_launch_counter() = 0;
    return h->run_fuser(false, (hipStream_t)st, inputs, n_inputs, token_dtype, N, ws, wsb, maps_out, tokens_out);
}

int gyre_op_seq_attn_max_len(int D) { return seq_attn_max_len(D); }
int gyre_op_seq_attn(void* st, const void* qkv, int ld_qkv, void* o, int ld_o, int N, int L, int heads, int D) {
    return launch_seq_attn((hipStream_t)st, (const bf16_t*)qkv, ld_qkv, (bf16_t*)o, ld_o, N, L, heads, D);
}
int gyre_op_quick_gelu(void* st, void* x, size_t n) { return launch_quick_gelu((hipStream_t)st, (bf16_t*)x, n); }
int gyre_op_fuser_pool(void* st, const void* x, int N, int C, size_t HW, void* out, int ld_out) {
    return launch_fuser_pool((hipStream_t)st, (const bf16_t*)x, N, C, HW, (bf16_t*)out, ld_out);
}
int gyre_op_fuser_gain(void* st, const void* x, const float* alpha, int ld_a, int N, int C, size_t HW, void* out, int accumulate) {
    return launch_fuser_gain((hipStream_t)st, (const bf16_t*)x, alpha, ld_a, N, C, HW, (bf16_t*)out, accumulate);
}

}  // extern "C"
