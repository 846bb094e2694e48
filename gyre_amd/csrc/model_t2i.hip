// T2I-adapter forward graphs (hint image -> one feature map per UNet down level) and their C ABI (include/gyre_hip.h).
//
// Topology restates the plain-torch adapters the reference vendors
//   gyre/pipeline/t2i_adapter/adapter.py:102-132   Adapter        ("main":  unshuffle, conv_in, levels x nums_rb ResnetBlock)
//   gyre/pipeline/t2i_adapter/adapter.py:240-263   Adapter_light  ("light": unshuffle, one extractor per level)
// driven once per request from gyre/pipeline/unified_pipeline.py:834-955; weights are addressed by the state-dict keys of those
// classes.  There is no normalisation, attention or time embedding: every layer is a 3x3 / 1x1 / stride-2 convolution on the GEMM
// kernels (Exec::conv3 / Exec::linear, bias and the residual add in their epilogues) plus the element-wise kernels of kernels_t2i.hip.
#include "model_impl.h"

namespace {
struct T2iConv { ConvW w; int k = 3; bool on = false; };
}  // namespace

struct gyre_t2i {
    gyre_t2i_cfg cfg;
    Store store;
    Exec ex;
    bool finalized = false;
    // main: conv_in, then body[level * nums_rb + j]
    struct Block { bool down = false; T2iConv down_op, in_conv, block1, block2, skep; };
    T2iConv conv_in;
    std::vector<Block> body;
    // light: one extractor per level
    struct Extractor { bool down = false; T2iConv in_conv, out_conv; std::vector<std::pair<T2iConv, T2iConv>> blocks; };
    std::vector<Extractor> ext;

    void reg(const std::string& key, int cout, int cin, int k, T2iConv& c) {
        c.k = k; c.on = true; c.w.cin = cin; c.w.cout = cout;
        c.w.w = k == 3 ? store.conv3(key, cout, cin, &c.w.b) : store.mat(key, cout, cin, true, true, &c.w.b);
    }
    int build() {
        const gyre_t2i_cfg& c = cfg;
        const int n = c.n_levels;
        if (c.kind != 0 && c.kind != 1) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "t2i: kind must be 0 (main) or 1 (light)");
        if (n < 1 || n > 4) GYRE_FAIL(GYRE_ERR_INVALID, "t2i: n_levels out of range");
        if (c.cin < 64 || c.cin % 64) GYRE_FAIL(GYRE_ERR_INVALID, "t2i: cin must be a positive multiple of 64 (PixelUnshuffle(8) of the image channels)");
        if (c.nums_rb < 1) GYRE_FAIL(GYRE_ERR_INVALID, "t2i: nums_rb must be positive");
        if (c.kind == 0 && c.ksize != 1 && c.ksize != 3) GYRE_FAIL(GYRE_ERR_INVALID, "t2i: ksize must be 1 or 3");
        for (int i = 0; i < n; ++i)
            if (c.channels[i] < 1 || (c.kind == 1 && c.channels[i] < 4)) GYRE_FAIL(GYRE_ERR_INVALID, "t2i: bad channel count");
        // adapter.py:87-99 hands skep the OUTPUT of in_conv although it was built for the block's input width: with sk == 0 the
        // reference itself only runs when every level has the same width
        if (c.kind == 0 && !c.sk)
            for (int i = 1; i < n; ++i)
                if (c.channels[i] != c.channels[0]) GYRE_FAIL(GYRE_ERR_UNSUPPORTED, "t2i: sk = 0 needs the same width at every level (as the reference's ResnetBlock does)");
        ex.store = &store;
        if (c.kind == 0) {
            reg("conv_in", c.channels[0], c.cin, 3, conv_in);
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < c.nums_rb; ++j) {
                    const std::string p = "body." + std::to_string(i * c.nums_rb + j);
                    Block b;
                    b.down = i != 0 && j == 0;
                    const int in_c = b.down ? c.channels[i - 1] : c.channels[i], out_c = c.channels[i];
                    if (in_c != out_c || !c.sk) reg(p + ".in_conv", out_c, in_c, c.ksize, b.in_conv);
                    reg(p + ".block1", out_c, out_c, 3, b.block1);
                    reg(p + ".block2", out_c, out_c, c.ksize, b.block2);
                    if (!c.sk) reg(p + ".skep", out_c, in_c, c.ksize, b.skep);
                    if (b.down && c.use_conv) reg(p + ".down_opt.op", in_c, in_c, 3, b.down_op);
                    body.push_back(b);
                }
        } else {
            for (int i = 0; i < n; ++i) {
                const std::string p = "body." + std::to_string(i);
                Extractor x;
                x.down = i != 0;
                const int in_c = i ? c.channels[i - 1] : c.cin, inter = c.channels[i] / 4;
                reg(p + ".in_conv", inter, in_c, 1, x.in_conv);
                for (int j = 0; j < c.nums_rb; ++j) {
                    x.blocks.emplace_back();
                    reg(p + ".body." + std::to_string(j) + ".block1", inter, inter, 3, x.blocks.back().first);
                    reg(p + ".body." + std::to_string(j) + ".block2", inter, inter, 3, x.blocks.back().second);
                }
                reg(p + ".out_conv", c.channels[i], inter, 1, x.out_conv);
                ext.push_back(x);
            }
        }
        for (void* a : store.allocs) if (!a) GYRE_FAIL(GYRE_ERR_HIP, "hipMalloc failed");
        return 0;
    }

    // y = conv(x) (+ residual): 3x3 with padding 1 (stride 1 or 2) or 1x1
    int conv(const Tn& x, const T2iConv& c, int stride, const Tn* residual, Tn& y) {
        if (c.k == 3) return ex.conv3(x, c.w, stride, 1, 0, nullptr, 0, residual, y);
        TRY(ex.alloc(y, x.B, x.H, x.W, pad8(c.w.cout)));
        return ex.linear(x.p, x.C, nullptr, 0, 0, x.rows(), x.C, c.w.w, y.C, c.w.b, residual ? residual->p : nullptr,
                         residual ? residual->C : 0, 0, y.p, y.C);
    }
    int pool(const Tn& x, Tn& y) {
        if (x.H < 2 || x.W < 2) GYRE_FAIL(GYRE_ERR_INVALID, "t2i: the image is too small for the adapter's downsampling levels");
        TRY(ex.alloc(y, x.B, x.H / 2, x.W / 2, x.C));
        return ex.dry() ? 0 : launch_avgpool2(ex.st, x.p, x.B, x.H, x.W, x.C, y.p);
    }
    // h = block2(relu(block1(x))) + res
    int two_convs(const Tn& x, const T2iConv& b1, const T2iConv& b2, const Tn& res, Tn& out) {
        Tn h;
        TRY(conv(x, b1, 1, nullptr, h));
        if (!ex.dry()) TRY(launch_relu(ex.st, h.p, (size_t)h.rows() * h.C));
        TRY(conv(h, b2, 1, &res, out));
        ex.free(h);
        return 0;
    }
    int emit(const Tn& f, int channels, void* out, int odt) {
        if (ex.dry()) return 0;
        if (!out) GYRE_FAIL(GYRE_ERR_INVALID, "t2i: null feature buffer");
        return launch_nhwc_to_nchw(ex.st, f.p, f.B, channels, f.H * f.W, f.C, out, odt);
    }

    int run(bool dry, hipStream_t st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb, void* const* outs, int odt) {
        const gyre_t2i_cfg& c = cfg;
        if (B < 1 || H < 8 || W < 8 || (H & 7) || (W & 7)) GYRE_FAIL(GYRE_ERR_INVALID, "t2i: H and W must be positive multiples of 8");
        ex.arena.reset((char*)ws, wsb, dry); ex.st = st; ex.batch = B; ex.cs_unit = 0;
        Tn x;
        TRY(ex.alloc(x, B, H / 8, W / 8, c.cin));
        if (!dry) TRY(launch_pixel_unshuffle8(st, img, idt, B, c.cin / 64, H, W, x.p));
        if (c.kind == 0) {
            Tn h;
            TRY(conv(x, conv_in, 1, nullptr, h));
            ex.free(x); x = h;
            for (int i = 0; i < c.n_levels; ++i) {
                for (int j = 0; j < c.nums_rb; ++j) {
                    const Block& b = body[i * c.nums_rb + j];
                    if (b.down) {
                        Tn d;
                        if (b.down_op.on) TRY(conv(x, b.down_op, 2, nullptr, d)); else TRY(pool(x, d));
                        ex.free(x); x = d;
                    }
                    if (b.in_conv.on) {
                        Tn t;
                        TRY(conv(x, b.in_conv, 1, nullptr, t));
                        ex.free(x); x = t;
                    }
                    Tn res = x, out;
                    if (b.skep.on) TRY(conv(x, b.skep, 1, nullptr, res));
                    TRY(two_convs(x, b.block1, b.block2, res, out));
                    if (b.skep.on) ex.free(res);
                    ex.free(x); x = out;
                }
                TRY(emit(x, c.channels[i], dry ? nullptr : outs[i], odt));
            }
        } else {
            for (int i = 0; i < c.n_levels; ++i) {
                const Extractor& e = ext[i];
                if (e.down) {
                    Tn d;
                    TRY(pool(x, d));
                    ex.free(x); x = d;
                }
                Tn t;
                TRY(conv(x, e.in_conv, 1, nullptr, t));
                ex.free(x); x = t;
                for (auto& rb : e.blocks) {
                    Tn out;
                    TRY(two_convs(x, rb.first, rb.second, x, out));
                    ex.free(x); x = out;
                }
                TRY(conv(x, e.out_conv, 1, nullptr, t));
                ex.free(x); x = t;
                TRY(emit(x, c.channels[i], dry ? nullptr : outs[i], odt));
            }
        }
        ex.free(x);
        return 0;
    }
};

extern "C" {

int gyre_t2i_create(const gyre_t2i_cfg* cfg, int device, gyre_t2i** out) { return handle_create(cfg, device, out); }
void gyre_t2i_destroy(gyre_t2i* h) { delete h; }
int gyre_t2i_num_params(const gyre_t2i* h) { return handle_num_params(h); }
const char* gyre_t2i_param_key(const gyre_t2i* h, int i) { return handle_param_key(h, i); }
int gyre_t2i_set_weight(gyre_t2i* h, const char* key, const void* p, int dtype, const int64_t* shape, int ndim, void* st) {
    return handle_set_weight(h, key, p, dtype, shape, ndim, st);
}
int gyre_t2i_finalize(gyre_t2i* h, void* st) { return handle_finalize(h); }
size_t gyre_t2i_workspace_bytes(gyre_t2i* h, int B, int H, int W) {
    if (!h) return 0;
    return h->run(true, nullptr, nullptr, 0, B, H, W, nullptr, 0, nullptr, 0) ? 0 : h->ex.arena.peak;
}
int gyre_t2i_forward(gyre_t2i* h, void* st, const void* img, int idt, int B, int H, int W, void* ws, size_t wsb,
                     void* const* features_out, int n, int odt) {
    if (!h || !img || !ws || !features_out) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    if (!h->finalized) GYRE_FAIL(GYRE_ERR_INCOMPLETE, "gyre_t2i_finalize has not succeeded");
    if (idt < 0 || idt > 2 || odt < 0 || odt > 2) GYRE_FAIL(GYRE_ERR_INVALID, "bad dtype");
    if (n != h->cfg.n_levels) GYRE_FAIL(GYRE_ERR_INVALID, "t2i: one feature buffer per level expected (" + std::to_string(h->cfg.n_levels) + ")");
    gyre_launch_counter() = 0;
    return h->run(false, (hipStream_t)st, img, idt, B, H, W, ws, wsb, features_out, odt);
}

int gyre_op_pixel_unshuffle8(void* st, const void* x, int dtype, int B, int c, int H, int W, void* y) {
    if (!x || !y) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    return launch_pixel_unshuffle8((hipStream_t)st, x, dtype, B, c, H, W, (bf16_t*)y);
}
int gyre_op_avgpool2(void* st, const void* x, int B, int H, int W, int C, void* y) {
    if (!x || !y) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    return launch_avgpool2((hipStream_t)st, (const bf16_t*)x, B, H, W, C, (bf16_t*)y);
}
int gyre_op_relu(void* st, void* x, size_t n) {
    if (!x) GYRE_FAIL(GYRE_ERR_INVALID, "null argument");
    return launch_relu((hipStream_t)st, (bf16_t*)x, n);
}

}  // extern "C"
