// RRDBNet (ESRGAN / Real-ESRGAN) upscaler graph and its C ABI (include/gyre_hip.h).
//
// Topology restates the published BasicSR RRDBNet (basicsr/archs/rrdbnet_arch.py: the reference imports it, gyre/pipeline/upscalers/
// upscaler_loader.py:7, but does not vendor it - *parity unpinned*) and the reference's own Plus block
// (gyre/pipeline/upscalers/models/esrgan_plus.py:29-47, eval mode: the Gaussian noise is the identity):
//   pixel_unshuffle by 2 / 4 for scale 2 / 1, conv_first, num_block RRDBs (three dense blocks each), feat + conv_body(body),
//   lrelu(conv_up1(nearest 2x)), lrelu(conv_up2(nearest 2x)), conv_last(lrelu(conv_hr)).
// Weights are addressed by BasicSR's state-dict names.
//
// Memory plan.  A dense block is ONE 192-channel NHWC buffer: x in channels [0, 64), x1 .. x4 in [64, 192); conv k reads the prefix
// [0, 32 + 32 k) and writes the next 32-channel slice, no concat is ever materialised.  Blocks ping-pong between two such buffers:
// conv5 writes channels [0, 64) of the other one, with the block's (and, for the third block of an RRDB, the RRDB's) residual
// arithmetic in its epilogue.  The RRDB input stays alive in a 64-channel side buffer for that last epilogue.
//
// Two paths for every 3x3 convolution, selectable per handle (gyre_rrdb_set_path):
//   generic  launch_gemm (the planner's tile kernels) with bias only, then k_rdb_epilogue in place over the written slice
//   fused    k_rdb_conv (kernels_rdb.hip): one launch, the epilogue applied to the fp32 accumulators, one rounding
// auto takes the fused kernel for the shape groups of RDB_AUTO_MASK: where it measured faster (profiles/upscaler_time.json).
// The weight record (UpConv) is the one of model_upscaler.h; the graph itself shares nothing with the window transformers.
#include "model_upscaler.h"

namespace {
struct RDense { UpConv c[5]; UpConv c1x1; };      // c1x1.w: the Plus block's 1x1, null without it

// Shape groups of the net's 3x3 convolutions, the unit the choice between the two paths is made in (and measured in:
// tools/upscaler_time.py turns them on one at a time through the tuning form of gyre_rrdb_set_path):
//   0  conv1 .. conv4 of a dense block    N = 32, Cin = 64 .. 160, body resolution
//   1  conv5 of a dense block             N = 64, Cin = 192
//   2  conv_up1, conv_up2                 N = 64, Cin = 64, nearest 2x in the gather
//   3  conv_last                          3 live channels, output resolution
//   4  conv_first, conv_body, conv_hr     N = 64, Cin <= 64, no upsample
int rdb_group(int Cin, int live, int ups) {
    if (ups) return 2;
    if (live <= 8) return 3;
    if (live <= 32) return 0;
    return Cin == 192 ? 1 : 4;
}
// auto: the groups whose fused time beat the generic path on the stacked 9 x 256 x 256 call (profiles/upscaler_time.json)
constexpr int RDB_AUTO_MASK = 0x1f;
constexpr int RDB_PATH_TUNING = 0x100;     // gyre_rrdb_set_path(0x100 | mask): fused exactly for the groups of the mask
}  // namespace

struct gyre_rrdb {
    gyre_rrdb_cfg cfg;
    Store store;
    Exec ex;
    bool finalized = false;
    int path = 0;                  // 0 auto, 1 generic, 2 fused, RDB_PATH_TUNING | group mask
    int r = 1, cin0 = 32;          // unshuffle factor and padded channels of the unshuffled image
    UpConv conv_first, conv_body, conv_up1, conv_up2, conv_hr, conv_last;
    std::vector<RDense> dense;     // 3 per RRDB

    void reg(const std::string& key, int cout, int cin, int cin_pad, UpConv& c) {
        c.cin = cin_pad; c.cout = cout; c.rows = pad8(cout);
        c.w = (bf16_t*)store.dmalloc((size_t)c.rows * 9 * cin_pad * 2, true);
        store.add(key + ".weight", {cout, cin, 3, 3}, PK_CONV3, c.w, c.rows, cin_pad);
        c.b = (float*)store.dmalloc((size_t)c.rows * 4, true);
        store.add(key + ".bias", {cout}, PK_VEC, c.b);
    }
    int build() {
        const gyre_rrdb_cfg& c = cfg;
        if (c.num_feat != 64 || c.num_grow_ch != 32)
            GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "rrdb: num_feat = 64 and num_grow_ch = 32 are the only widths built (every configuration of the reference)");
        if (c.scale != 1 && c.scale != 2 && c.scale != 4) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "rrdb: scale must be 1, 2 or 4");
        if (c.num_in_ch < 1 || c.num_in_ch > 4 || c.num_out_ch < 1 || c.num_out_ch > 8) GYRE_FAIL(GYRE_ERR_INVALID, "rrdb: 1 to 4 input and 1 to 8 output channels");
        if (c.num_block < 1 || c.num_block > 64) GYRE_FAIL(GYRE_ERR_INVALID, "rrdb: num_block out of range");
        r = c.scale == 2 ? 2 : c.scale == 1 ? 4 : 1;
        cin0 = rdb_unshuffle_channels(c.num_in_ch, r);
        ex.store = &store;
        reg("conv_first", 64, c.num_in_ch * r * r, cin0, conv_first);
        for (int i = 0; i < c.num_block; ++i)
            for (int j = 1; j <= 3; ++j) {
                const std::string p = "body." + std::to_string(i) + ".rdb" + std::to_string(j);
                RDense d;
                for (int k = 0; k < 5; ++k) reg(p + ".conv" + std::to_string(k + 1), k == 4 ? 64 : 32, 64 + 32 * k, 64 + 32 * k, d.c[k]);
                if (c.plus) {
                    d.c1x1.cin = 64; d.c1x1.cout = 32; d.c1x1.rows = 32;
                    d.c1x1.w = store.mat(p + ".conv1x1", 32, 64, true, false, nullptr);
                }
                dense.push_back(d);
            }
        reg("conv_body", 64, 64, 64, conv_body);
        reg("conv_up1", 64, 64, 64, conv_up1);
        reg("conv_up2", 64, 64, 64, conv_up2);
        reg("conv_hr", 64, 64, 64, conv_hr);
        reg("conv_last", c.num_out_ch, 64, 64, conv_last);
        for (void* a : store.allocs) if (!a) GYRE_FAIL(GYRE_ERR_HIP, "hipMalloc failed");
        return 0;
    }

    // slice pointer; a dry run plans with aligned stand-ins of the same residue mod 256 (arena tensors are 256-byte aligned)
    bf16_t* at(const Tn& t, int c0) const { return ex.arena.dry ? (bf16_t*)(uintptr_t)(4096 + 2 * c0) : t.p + c0; }
    bool fused(const UpConv& c, int Cin, int ups) const {
        if (path == 1 || path == 2) return path == 2;
        const int mask = path & RDB_PATH_TUNING ? path & 0x1f : RDB_AUTO_MASK;
        return (mask >> rdb_group(Cin, c.cout, ups)) & 1;
    }
    // out[pix][c0 .. c0 + cout) = epilogue(conv3x3(x[pix][0 .. Cin))), x NHWC [B][H][W] with pixel stride x.C
    int conv(const Tn& x, int Cin, int ups, const UpConv& c, Tn& out, int c0, RdbEpilogueArgs e) {
        if (Cin != c.cin || Cin > x.C || c0 + c.rows > out.C) GYRE_FAIL(GYRE_ERR_INVALID, "rrdb: internal shape mismatch");
        const int Ho = ups ? 2 * x.H : x.H, Wo = ups ? 2 * x.W : x.W;
        if (out.H != Ho || out.W != Wo || out.B != x.B) GYRE_FAIL(GYRE_ERR_INVALID, "rrdb: internal size mismatch");
        if (fused(c, Cin, ups)) {
            if (ex.dry()) return 0;
            const int NT = c.rows <= 32 ? 32 : 64;
            bool fresh = false;
            bf16_t* wd = (bf16_t*)store.derived(Store::DC_RDB_CHUNKED, c.w, rdb_wpack_bytes(NT, Cin), &fresh, NT);
            if (!wd) GYRE_FAIL(GYRE_ERR_HIP, "cannot allocate the chunk-ordered weight copy of the dense-block convolution");
            if (!fresh) TRY(launch_rdb_wpack(ex.st, c.w, c.rows, Cin, NT, wd));
            e.bias = c.b;
            return launch_rdb_conv(ex.st, x.p, x.C, Cin, x.B, x.H, x.W, ups, wd, NT, c.cout, out.p + c0, out.C, e);
        }
        GemmParams p;
        p.A = at(x, 0); p.lda = x.C; p.mode = GEMM_CONV3;
        p.Hi = x.H; p.Wi = x.W; p.Cin = Cin; p.Ho = Ho; p.Wo = Wo; p.stride = 1; p.pad = 1; p.ups = ups;
        p.Hup = ups ? Ho : 0; p.Wup = ups ? Wo : 0;
        p.W = c.w; p.K = 9 * Cin; p.N = c.rows; p.M = x.B * Ho * Wo;
        p.bias = c.b; p.rows_per_sample = Ho * Wo;
        p.out = at(out, c0); p.ldc = out.C; p.out_mode = OUT_BF16;
        TRY(ex.run_gemm(p));
        if (ex.dry() || (e.alpha == 1.f && !e.act && !e.r1 && !e.r2)) return 0;
        e.bias = nullptr;                                   // (the GEMM added it)
        return launch_rdb_epilogue(ex.st, out.p + c0, out.C, c.cout, (size_t)x.B * Ho * Wo, e);
    }
    static RdbEpilogueArgs act_only() { RdbEpilogueArgs e; e.act = 1; return e; }

    // one dense block: x = cur[0:64) -> nxt[0:64); rrdb_in != null: the third block of an RRDB
    int dense_block(const RDense& d, Tn& cur, Tn& nxt, const Tn* rrdb_in) {
        for (int k = 0; k < 4; ++k) {
            RdbEpilogueArgs e = act_only();
            Tn tmp;
            if (k == 1 && d.c1x1.w) {
                // Plus: x2 = lrelu(conv2(x | x1)) + conv1x1(x).  Fused: the 1x1 lands in the x2 slice and conv2 adds it in place (r1 aliases
                // the output); generic: the GEMM would overwrite the slice first, so the 1x1 goes to a side tensor
                const bool inplace = fused(d.c[1], 96, 0);
                bf16_t* dst; int ldd;
                if (inplace) { dst = at(cur, 96); ldd = cur.C; }
                else { TRY(ex.alloc(tmp, cur.B, cur.H, cur.W, 32)); dst = at(tmp, 0); ldd = 32; }
                TRY(ex.linear(at(cur, 0), cur.C, nullptr, 0, 0, cur.rows(), 64, d.c1x1.w, 32, nullptr, nullptr, 0, 0, dst, ldd));
                e.r1 = dst; e.ldr1 = ldd; e.beta1 = 1.f;
            }
            TRY(conv(cur, 64 + 32 * k, 0, d.c[k], cur, 64 + 32 * k, e));
            if (tmp.valid()) ex.free(tmp);
        }
        RdbEpilogueArgs e;
        e.alpha = rrdb_in ? 0.04f : 0.2f;
        e.r1 = at(cur, 0); e.ldr1 = cur.C; e.beta1 = rrdb_in ? 0.2f : 1.f;
        if (rrdb_in) { e.r2 = at(*rrdb_in, 0); e.ldr2 = rrdb_in->C; e.beta2 = 1.f; }
        return conv(cur, 192, 0, d.c[4], nxt, 0, e);
    }

    int run(bool dry, hipStream_t st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
        const gyre_rrdb_cfg& c = cfg;
        if (B < 1 || H < r || W < r || H % r || W % r)
            GYRE_FAIL(GYRE_ERR_INVALID, "rrdb: H and W must be positive multiples of " + std::to_string(r) + " for scale " + std::to_string(c.scale));
        ex.arena.reset((char*)ws, wsb, dry); ex.st = st; ex.batch = B; ex.cs_unit = 0;
        const int h = H / r, w = W / r;
        Tn x0, feat, side, a, b;
        TRY(ex.alloc(x0, B, h, w, cin0));
        if (!dry) TRY(launch_pixel_unshuffle(st, img, idt, B, c.num_in_ch, H, W, r, x0.p));
        TRY(ex.alloc(feat, B, h, w, 64));
        TRY(conv(x0, cin0, 0, conv_first, feat, 0, RdbEpilogueArgs()));
        ex.free(x0);
        TRY(ex.alloc(a, B, h, w, 192));
        TRY(ex.alloc(b, B, h, w, 192));
        TRY(ex.alloc(side, B, h, w, 64));
        const size_t npix = (size_t)B * h * w;
        if (!dry) TRY(launch_rdb_copy(st, feat.p, 64, a.p, 192, 64, npix));
        Tn* cur = &a; Tn* nxt = &b;
        for (int i = 0; i < c.num_block; ++i) {
            const Tn* rin = &feat;                               // the first RRDB's input is conv_first's output, which stays alive
            if (i > 0) { rin = &side; if (!dry) TRY(launch_rdb_copy(st, cur->p, 192, side.p, 64, 64, npix)); }
            for (int j = 0; j < 3; ++j) {
                TRY(dense_block(dense[3 * i + j], *cur, *nxt, j == 2 ? rin : nullptr));
                std::swap(cur, nxt);
            }
        }
        ex.free(side);
        Tn body;
        TRY(ex.alloc(body, B, h, w, 64));
        {
            RdbEpilogueArgs e;
            e.r1 = at(feat, 0); e.ldr1 = 64; e.beta1 = 1.f;        // feat + conv_body(body)
            TRY(conv(*cur, 64, 0, conv_body, body, 0, e));
        }
        ex.free(a); ex.free(b); ex.free(feat);
        Tn u1, u2, hr, last;
        TRY(ex.alloc(u1, B, 2 * h, 2 * w, 64));
        TRY(conv(body, 64, 1, conv_up1, u1, 0, act_only()));
        ex.free(body);
        TRY(ex.alloc(u2, B, 4 * h, 4 * w, 64));
        TRY(conv(u1, 64, 1, conv_up2, u2, 0, act_only()));
        ex.free(u1);
        TRY(ex.alloc(hr, B, 4 * h, 4 * w, 64));
        TRY(conv(u2, 64, 0, conv_hr, hr, 0, act_only()));
        ex.free(u2);
        TRY(ex.alloc(last, B, 4 * h, 4 * w, conv_last.rows));
        TRY(conv(hr, 64, 0, conv_last, last, 0, RdbEpilogueArgs()));
        ex.free(hr);
        if (!dry) {
            if (!out) GYRE_FAIL(GYRE_ERR_INVALID, "rrdb: null output buffer");
            TRY(launch_nhwc_to_nchw(st, last.p, B, c.num_out_ch, 16 * h * w, last.C, out, odt));
        }
        ex.free(last);
        return 0;
    }
};

extern "C" {

int gyre_rrdb_create(const gyre_rrdb_cfg* cfg, int device, gyre_rrdb** out) { return handle_create(cfg, device, out); }
void gyre_rrdb_destroy(gyre_rrdb* h) { delete h; }
int gyre_rrdb_num_params(const gyre_rrdb* h) { return handle_num_params(h); }
const char* gyre_rrdb_param_key(const gyre_rrdb* h, int i) { return handle_param_key(h, i); }
int gyre_rrdb_set_weight(gyre_rrdb* h, const char* key, const void* p, int dtype, const int64_t* shape, int ndim, void* st) {
    return handle_set_weight(h, key, p, dtype, shape, ndim, st);
}
int gyre_rrdb_finalize(gyre_rrdb* h, void* st) { return handle_finalize(h); }
int gyre_rrdb_set_path(gyre_rrdb* h, int path) {
    if (!h) GYRE_FAIL(GYRE_ERR_INVALID, "null handle");
    if ((path < 0 || path > 2) && (path & ~0x1f) != RDB_PATH_TUNING)
        GYRE_FAIL(GYRE_ERR_INVALID, "rrdb: path must be 0 (auto), 1 (generic), 2 (fused) or 0x100 | a mask of the five shape groups");
    h->path = path;
    return 0;
}
size_t gyre_rrdb_workspace_bytes(gyre_rrdb* h, int B, int H, int W) { return handle_workspace_bytes(h, B, H, W); }
int gyre_rrdb_forward(gyre_rrdb* h, void* st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* out, int odt) {
    return handle_forward(h, "rrdb", st, img, idt, B, H, W, ws, wsb, out, odt);
}

int gyre_op_rdb_tile(int* th, int* tw) {
    if (!th || !tw) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    rdb_tile(th, tw);
    return 0;
}
static RdbEpilogueArgs rdb_epi_from(const gyre_rdb_epilogue& e) {
    RdbEpilogueArgs a;
    a.bias = e.bias; a.alpha = e.alpha; a.act = e.act;
    a.r1 = (const bf16_t*)e.r1; a.ldr1 = e.ldr1; a.beta1 = e.beta1; a.r2 = (const bf16_t*)e.r2; a.ldr2 = e.ldr2; a.beta2 = e.beta2;
    return a;
}
int gyre_op_rdb_conv(void* st, const gyre_rdb_conv_args* a) {
    if (!a || !a->x || !a->w || !a->out || !a->wpack || !a->epi) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    if (a->c0 < 0 || a->ldo < a->c0 + a->N_live) GYRE_FAIL(GYRE_ERR_INVALID, "rdb_conv: the slice [c0, c0 + N_live) must lie inside the pixel stride ldo");
    if (a->c0 % 8) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "rdb_conv: the slice offset must be a multiple of 8 channels");
    // every refusal of the launch comes before the first write: a refused call leaves the output AND the weight scratch untouched
    const RdbEpilogueArgs e = rdb_epi_from(*a->epi);
    TRY(rdb_conv_check((const bf16_t*)a->x, a->ldx, a->Cin, a->B, a->H, a->W, a->ups, (const bf16_t*)a->wpack, a->NT, a->N_live,
                       (const bf16_t*)a->out + a->c0, a->ldo, e));
    if (a->w_rows < 1 || a->w_rows > a->NT) GYRE_FAIL(GYRE_ERR_INVALID, "rdb_conv: 1 to NT weight rows");
    if ((size_t)a->w & 15) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "rdb_conv: the weights must be 16-byte aligned");
    if (a->wpack_bytes < rdb_wpack_bytes(a->NT, a->Cin)) GYRE_FAIL(GYRE_ERR_WORKSPACE, "rdb_conv: the weight scratch is too small");
    TRY(launch_rdb_wpack((hipStream_t)st, (const bf16_t*)a->w, a->w_rows, a->Cin, a->NT, (bf16_t*)a->wpack));
    return launch_rdb_conv((hipStream_t)st, (const bf16_t*)a->x, a->ldx, a->Cin, a->B, a->H, a->W, a->ups, (const bf16_t*)a->wpack, a->NT,
                           a->N_live, (bf16_t*)a->out + a->c0, a->ldo, e);
}
int gyre_op_rdb_epilogue(void* st, void* x, int c0, int ldo, int N_live, size_t npix, const gyre_rdb_epilogue* e) {
    if (!x || !e) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    if (c0 < 0 || ldo < c0 + N_live) GYRE_FAIL(GYRE_ERR_INVALID, "rdb_epilogue: the slice [c0, c0 + N_live) must lie inside the pixel stride ldo");
    if (c0 % 8) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "rdb_epilogue: the slice offset must be a multiple of 8 channels");
    return launch_rdb_epilogue((hipStream_t)st, (bf16_t*)x + c0, ldo, N_live, npix, rdb_epi_from(*e));
}
int gyre_op_pixel_unshuffle(void* st, const void* x, int dtype, int B, int c, int H, int W, int r, void* y) {
    return launch_pixel_unshuffle((hipStream_t)st, x, dtype, B, c, H, W, r, (bf16_t*)y);
}

}  // extern "C"
