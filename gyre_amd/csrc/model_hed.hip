// The HED edge-detector graph and its C ABI (include/gyre_hip.h): the reference's HED (gyre/pipeline/hinters/models/hed.py, the
// holistically-nested edge detector on a VGG-16 trunk), which it serves as hinters-hed / hinters-hed-alt behind HedPipeline.
//
// Topology, every activation NHWC in the storage type, every score fp32:
//   entry     NCHW image -> [B][H + 68][W + 68][8], the image inside a 34-pixel zero border (k_hed_entry): conv1_1's padding 35 is that
//             border plus the planner's ordinary padding 1, so stage 1 works at (H + 68) x (W + 68)
//   stage k   2, 2, 3, 3, 3 planner convolutions 3x3 / pad 1 of 64, 128, 256, 512, 512 channels; the ReLU of every convolution but the
//             stage's last is the in-place launch_relu
//   tail k    one read of the stage's last convolution before its ReLU (k_hed_tail): the next stage's input, relu(max) over the 2x2
//             ceil-mode window (H_{k+1} = ceil(H_k / 2); not written for stage 5), and the side score score_dsn_k, a 1x1 convolution to
//             one channel of the ReLU output, [B][H_k][W_k] fp32.  The full-resolution ReLU tensor is never written
//   fuse      per output pixel (k_hed_fuse): so1 cropped; so2 .. so5 through their bilinear transposed convolution (kernel 2 s, stride
//             s = 2^(k-1), output (H_k + 1) s) evaluated in place and cropped; score_final over the five; six sigmoids; out [6][B][1][H][W]
// Crop offsets: the reference's crop() takes int(round(d / 2.)) of the size difference d - Python's round, half to even.  They are
// computed here (crop_offset) and handed to the kernel as integers; d is odd for every odd H or W.
//
// The planner sees every launch as if its sample ran alone (BatchInvariantScope) and the tail's sums have an order that depends on the
// channel count alone: a sample's result does not depend on the batch it runs in.
#include "model_upscaler.h"

namespace {
constexpr int HED_STAGES = 5;
constexpr int HED_CONVS[HED_STAGES] = {2, 2, 3, 3, 3};
constexpr int HED_WIDTH[HED_STAGES] = {64, 128, 256, 512, 512};

// Python's int(round(d / 2.)): halves go to the even neighbour
inline int crop_offset(long long d) {
    const long long q = d / 2;                        // d >= 0
    return (int)((d & 1) ? q + (q & 1) : q);
}
// stage sizes of an image side n: n + 68, then ceil halves
inline void stage_sizes(int n, int* s) {
    s[0] = n + 2 * HED_BORDER;
    for (int k = 1; k < HED_STAGES; ++k) s[k] = (s[k - 1] + 1) / 2;
}
// crop offsets of the five maps for an image side n
inline void crop_offsets(int n, const int* s, int* o) {
    o[0] = crop_offset((long long)s[0] - n);
    for (int k = 1; k < HED_STAGES; ++k) o[k] = crop_offset((((long long)s[k] + 1) << k) - n);
}
}  // namespace

struct gyre_hed {
    gyre_hed_cfg cfg;
    Store store;
    Exec ex;
    bool finalized = false;
    UpConv conv[13];
    float *sw[HED_STAGES] = {}, *sb[HED_STAGES] = {}, *fw = nullptr, *fb = nullptr;      // score_dsn1..5, score_final: fp32 vectors

    void conv3reg(const std::string& key, int cout, int cin, int cin_pad, UpConv& c) {
        c.cin = cin_pad; c.cout = cout; c.rows = cout;
        c.w = (bf16_t*)store.dmalloc((size_t)cout * 9 * cin_pad * 2, true);
        store.add(key + ".weight", {cout, cin, 3, 3}, PK_CONV3, c.w, cout, cin_pad);
        c.b = (float*)store.dmalloc((size_t)cout * 4, true);
        store.add(key + ".bias", {cout}, PK_VEC, c.b);
    }
    // a 1x1 convolution to one channel, kept as fp32 vectors (the kernels read them as such)
    void scorereg(const std::string& key, int cin, float** w, float** b) {
        *w = (float*)store.dmalloc((size_t)pad8(cin) * 4, true);
        store.add(key + ".weight", {1, cin, 1, 1}, PK_TABLE_F32, *w);
        *b = (float*)store.dmalloc(16, true);
        store.add(key + ".bias", {1}, PK_TABLE_F32, *b);
    }
    int build() {
        if (cfg.reserved != 0) GYRE_FAIL(GYRE_ERR_INVALID, "hed: the reserved configuration field must be 0");
        ex.store = &store;
        int n = 0, cin = 3;
        for (int k = 0; k < HED_STAGES; ++k)
            for (int j = 0; j < HED_CONVS[k]; ++j) {
                conv3reg("conv" + std::to_string(k + 1) + "_" + std::to_string(j + 1), HED_WIDTH[k], cin, cin == 3 ? 8 : cin, conv[n++]);
                cin = HED_WIDTH[k];
            }
        for (int k = 0; k < HED_STAGES; ++k) scorereg("score_dsn" + std::to_string(k + 1), HED_WIDTH[k], &sw[k], &sb[k]);
        scorereg("score_final", 5, &fw, &fb);
        for (void* a : store.allocs) if (!a) GYRE_FAIL(GYRE_ERR_HIP, "hipMalloc failed");
        return 0;
    }

    bf16_t* at(const Tn& t) const { return ex.arena.dry ? (bf16_t*)(uintptr_t)4096 : t.p; }
    // out = conv3x3(x) + bias, zero padding 1, on the planner
    int conv3(const Tn& x, const UpConv& c, Tn& out) {
        if (x.C != c.cin || out.C != c.rows || out.H != x.H || out.W != x.W || out.B != x.B) GYRE_FAIL(GYRE_ERR_INVALID, "hed: internal shape mismatch");
        GemmParams p;
        p.A = at(x); p.lda = x.C; p.mode = GEMM_CONV3;
        p.Hi = x.H; p.Wi = x.W; p.Cin = x.C; p.Ho = x.H; p.Wo = x.W; p.stride = 1; p.pad = 1; p.ups = 0;
        p.W = c.w; p.K = 9 * x.C; p.N = c.rows; p.M = x.B * x.H * x.W;
        p.bias = c.b; p.rows_per_sample = x.H * x.W;
        p.out = at(out); p.ldc = out.C; p.out_mode = OUT_BF16;
        return ex.run_gemm(p);
    }

    int run(bool dry, hipStream_t st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
        if (B < 1 || B > 65535 || H < 1 || W < 1) GYRE_FAIL(GYRE_ERR_INVALID, "hed: the image must be at least 1 x 1, the batch 1 to 65535");
        // the planner indexes rows with 32-bit integers: stage 1 has B (H + 68)(W + 68) of them
        if (H > 0x3fffffff - 2 * HED_BORDER || W > 0x3fffffff - 2 * HED_BORDER ||
            (size_t)B * (H + 2 * HED_BORDER) * (W + 2 * HED_BORDER) > 0x3fffffff)
            GYRE_FAIL(GYRE_ERR_INVALID, "hed: image too large (B (H + 68) (W + 68) must stay below 2^30)");
        BatchInvariantScope invariant;
        ex.arena.reset((char*)ws, wsb, dry); ex.st = st; ex.batch = B; ex.cs_unit = 0;
        int hs[HED_STAGES], wsz[HED_STAGES];
        stage_sizes(H, hs); stage_sizes(W, wsz);
        Tn cur, nxt, so[HED_STAGES];
        TRY(ex.alloc(cur, B, hs[0], wsz[0], 8));
        if (!dry) TRY(launch_hed_entry(st, img, idt, B, H, W, cur.p));
        int n = 0;
        for (int k = 0; k < HED_STAGES; ++k) {
            for (int j = 0; j < HED_CONVS[k]; ++j) {
                TRY(ex.alloc(nxt, B, hs[k], wsz[k], HED_WIDTH[k]));
                TRY(conv3(cur, conv[n++], nxt));
                ex.free(cur);
                cur = nxt; nxt = Tn();
                if (j + 1 < HED_CONVS[k] && !dry) TRY(launch_relu(st, cur.p, (size_t)cur.rows() * cur.C));
            }
            TRY(ex.alloc_raw(so[k], (size_t)B * hs[k] * wsz[k] * sizeof(float)));
            const bool pool = k + 1 < HED_STAGES;
            if (pool) TRY(ex.alloc(nxt, B, hs[k + 1], wsz[k + 1], HED_WIDTH[k]));
            if (!dry) TRY(launch_hed_tail(st, cur.p, B, hs[k], wsz[k], HED_WIDTH[k], sw[k], sb[k], pool ? nxt.p : nullptr, (float*)so[k].p));
            ex.free(cur);
            cur = nxt; nxt = Tn();
        }
        if (!dry) {
            if (!out) GYRE_FAIL(GYRE_ERR_INVALID, "hed: null output buffer");
            HedFuse a;
            crop_offsets(H, hs, a.oy); crop_offsets(W, wsz, a.ox);
            for (int k = 0; k < HED_STAGES; ++k) { a.so[k] = (const float*)so[k].p; a.Hk[k] = hs[k]; a.Wk[k] = wsz[k]; }
            a.wf = fw; a.bf = fb; a.out = out; a.out_dtype = odt; a.B = B; a.H = H; a.W = W;
            TRY(launch_hed_fuse(st, a));
        }
        for (int k = 0; k < HED_STAGES; ++k) ex.free(so[k]);
        return 0;
    }
};

extern "C" {

int gyre_hed_create(const gyre_hed_cfg* cfg, int device, gyre_hed** out) { return handle_create(cfg, device, out); }
void gyre_hed_destroy(gyre_hed* h) { delete h; }
int gyre_hed_num_params(const gyre_hed* h) { return handle_num_params(h); }
const char* gyre_hed_param_key(const gyre_hed* h, int i) { return handle_param_key(h, i); }
int gyre_hed_set_weight(gyre_hed* h, const char* key, const void* p, int dtype, const int64_t* shape, int ndim, void* st) {
    return handle_set_weight(h, key, p, dtype, shape, ndim, st);
}
int gyre_hed_finalize(gyre_hed* h, void* st) { return handle_finalize(h); }
size_t gyre_hed_workspace_bytes(gyre_hed* h, int B, int H, int W) { return handle_workspace_bytes(h, B, H, W); }
int gyre_hed_forward(gyre_hed* h, void* st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
    return handle_forward(h, "hed", st, img, idt, B, H, W, ws, wsb, out, odt);
}
// the geometry the graph uses for an image side n: sizes[5] of the stages, offsets[5] of the crops
int gyre_hed_geometry(int n, int32_t* sizes, int32_t* offsets) {
    if (n < 1 || n > 0x3fffffff - 2 * HED_BORDER || !sizes || !offsets) GYRE_FAIL(GYRE_ERR_INVALID, "hed_geometry: a side of at least 1 and two arrays of 5");
    int s[HED_STAGES], o[HED_STAGES];
    stage_sizes(n, s); crop_offsets(n, s, o);
    for (int k = 0; k < HED_STAGES; ++k) { sizes[k] = s[k]; offsets[k] = o[k]; }
    return 0;
}

// ---- test hooks of kernels_hed.hip ----
int gyre_op_hed_entry(void* st, const void* x, int dtype, int B, int H, int W, void* y) {
    return launch_hed_entry((hipStream_t)st, x, dtype, B, H, W, (bf16_t*)y);
}
int gyre_op_hed_tail(void* st, const void* x, int B, int Hs, int Ws, int C, const float* w, const float* bias, void* pool, float* so) {
    return launch_hed_tail((hipStream_t)st, (const bf16_t*)x, B, Hs, Ws, C, w, bias, (bf16_t*)pool, so);
}
int gyre_op_hed_fuse(void* st, const gyre_hed_fuse_args* g) {
    if (!g) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    HedFuse a;
    for (int k = 0; k < HED_STAGES; ++k) { a.so[k] = g->so[k]; a.Hk[k] = g->Hk[k]; a.Wk[k] = g->Wk[k]; a.oy[k] = g->oy[k]; a.ox[k] = g->ox[k]; }
    a.wf = g->wf; a.bf = g->bf; a.out = g->out; a.out_dtype = g->out_dtype; a.B = g->B; a.H = g->H; a.W = g->W;
    return launch_hed_fuse((hipStream_t)st, a);
}

}  // extern "C"
