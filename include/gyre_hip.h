/*
 * gyre_hip.h - C ABI of libgyre_hip.so, the MI355X (gfx950) native UNet / VAE
 * for Gyre's diffusion generation path.
 *
 * Nothing like this exists in the reference (it is pure Python and crosses into
 * third-party diffusers modules); each entry point below replaces one of the
 * reference's Python call sites across that boundary:
 *
 *   gyre_unet_forward     <- gyre/pipeline/unet/core.py:262-274
 *                            `self.unet(latents, t, encoder_hidden_states=...).sample`
 *                            (Protocol gyre/pipeline/unet/types.py:26-39)
 *   gyre_vae_encode       <- gyre/pipeline/unified_pipeline.py:309
 *                            `self.pipeline.vae.encode(image).latent_dist`  (returns the moments;
 *                            the per-generator posterior sample :311-313 stays host PyTorch)
 *   gyre_vae_decode       <- gyre/pipeline/unified_pipeline.py:1531-1533  `self.vae.decode(latents).sample`
 *   gyre_*_create         <- gyre/manager.py:1068-1112  `Class(**config)`
 *   gyre_*_set_weight     <- gyre/manager.py:1068-1112  `load_state_dict` (keys = diffusers names,
 *                            the key space gyre/ckpt_utils.py:259-285 produces)
 *   gyre_*_destroy        <- gyre/pipeline/pipeline_wrapper.py:144-158 deactivate()
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer marked "dev" is a device pointer
 *     valid on the handle's device.  No torch / C++ types cross this boundary.
 *   - every function returns 0 on success or a negative gyre_status; on failure
 *     gyre_last_error() (thread-local) holds a message.  Nothing throws.
 *   - all work is enqueued on the hipStream_t passed as `stream` (void* here so the
 *     header needs no HIP include).  No function calls hipDeviceSynchronize; the
 *     caller owns synchronisation.  Handles hold no global mutable state: different
 *     handles may be used concurrently from different threads (one in-flight call
 *     per handle, the reference's one-thread-per-device-slot rule,
 *     gyre/manager.py:2107-2139).
 *   - activations cross the boundary in the reference's own layout: NCHW for
 *     latents/images, [B,S,D] for text embeddings; dtype per call (gyre_dtype).
 *     Internally everything is NHWC bf16 (libgyre_hip.so) or NHWC fp16 (libgyre_hip_f16.so, gyre_storage_dtype) with fp32
 *     accumulation.
 *   - `workspace` is caller-allocated device scratch (e.g. from the torch caching
 *     allocator) of at least gyre_*_workspace_bytes(...) bytes, 256-byte aligned.
 */
#ifndef GYRE_HIP_H
#define GYRE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GYRE_ABI_VERSION 1

typedef enum { GYRE_F32 = 0, GYRE_BF16 = 1, GYRE_F16 = 2 } gyre_dtype;

typedef enum {
    GYRE_OK = 0,
    GYRE_ERR_INVALID = -1,     /* bad argument / shape / dtype            -> Python ValueError */
    GYRE_ERR_KEY = -2,         /* unknown or shape-mismatched weight key -> Python KeyError   */
    GYRE_ERR_INCOMPLETE = -3,  /* forward before every weight was set    -> RuntimeError      */
    GYRE_ERR_WORKSPACE = -4,   /* workspace too small                    -> RuntimeError      */
    GYRE_ERR_HIP = -5,         /* a HIP runtime call failed              -> RuntimeError      */
    GYRE_ERR_UNSUPPORTED = -6  /* configuration not implemented          -> NotImplementedError */
} gyre_status;

#define GYRE_MAX_LEVELS 8

/* Mirrors the diffusers UNet2DConditionModel config.json fields the reference
 * relies on (SD1.x values from gyre/ldm_config/v1-inference.yaml:29-47). */
typedef struct {
    int32_t in_channels;             /* 4, or 9 for the runway inpaint UNet (unified_pipeline.py:668-690) */
    int32_t out_channels;            /* 4 */
    int32_t n_levels;                /* 4 */
    int32_t block_out_channels[GYRE_MAX_LEVELS]; /* 320,640,1280,1280 */
    int32_t layers_per_block;        /* 2 */
    int32_t attn_levels[GYRE_MAX_LEVELS];        /* 1,1,1,0 */
    int32_t num_heads[GYRE_MAX_LEVELS];          /* 8,8,8,8 */
    int32_t transformer_depth[GYRE_MAX_LEVELS];  /* 1,1,1,1 */
    int32_t cross_attention_dim;     /* 768 */
    int32_t norm_num_groups;         /* 32 */
    int32_t use_linear_projection;   /* 0 for SD1.x */
    int32_t flip_sin_to_cos;         /* 1 */
    float   freq_shift;              /* 0 */
} gyre_unet_cfg;

typedef struct {
    int32_t in_channels;             /* 3 */
    int32_t out_channels;            /* 3 */
    int32_t latent_channels;         /* 4 */
    int32_t n_levels;                /* 4 */
    int32_t block_out_channels[GYRE_MAX_LEVELS]; /* 128,256,512,512 */
    int32_t layers_per_block;        /* 2 */
    int32_t norm_num_groups;         /* 32 */
} gyre_vae_cfg;

/* T2I adapter (reference gyre/pipeline/t2i_adapter/adapter.py: Adapter = "main", Adapter_light = "light") */
typedef struct {
    int32_t kind;                    /* 0 main, 1 light */
    int32_t cin;                     /* 64 x image channels (PixelUnshuffle(8)): 64 or 192 */
    int32_t channels[4];             /* 320,640,1280,1280 */
    int32_t n_levels;                /* 4 */
    int32_t nums_rb;                 /* residual blocks per level: 2 (main), 4 (light) */
    int32_t ksize;                   /* main: kernel size of in_conv / block2 / skep, 1 or 3 */
    int32_t sk;                      /* main: 1 = identity skip (no skep conv, in_conv only where the width changes) */
    int32_t use_conv;                /* main: 1 = stride-2 conv downsampling (down_opt.op), 0 = 2x2 average pool */
} gyre_t2i_cfg;

/* Token-sequence T2I networks (reference gyre/pipeline/t2i_adapter/adapter.py: StyleAdapter, CoAdapterFuser): pre-LN transformers of
 * n_layers ResidualAttentionBlocks of `width` channels and num_head heads; width / num_head must be 32, 64, 96 or 128
 * (GYRE_ERR_UNSUPPORTED at create otherwise). */
enum { GYRE_T2I_SEQ_STYLE = 0, GYRE_T2I_SEQ_FUSER = 1 };
typedef struct {
    int32_t kind;                    /* GYRE_T2I_SEQ_STYLE / GYRE_T2I_SEQ_FUSER */
    int32_t width;                   /* 1024 (style), 768 (fuser) */
    int32_t num_head;                /* 8 */
    int32_t n_layers;                /* 3 (the reference spells it n_layes) */
    int32_t num_token;               /* style: rows of style_embedding = tokens returned, 8 */
    int32_t context_dim;             /* style: columns of proj, 768 */
    int32_t unet_channels[4];        /* fuser: 320,640,1280,1280 (multiples of 8) */
} gyre_t2i_seq_cfg;
/* One entry of the fuser's ordered input (the reference's `features` dict): the ExtraCondition index of the co-adapter (sketch 0,
 * keypose 1, seg 2, depth 3, canny 4, style 5, color 6, openpose 7) and either its four spatial states - tokens == 0, in[i] NCHW
 * [N][unet_channels[i]][h[i]][w[i]] in the STORAGE type - or one token tensor - tokens = T > 0, in[0] [N][T][width] of the call's
 * token dtype. */
typedef struct {
    int32_t task;
    int32_t tokens;
    const void* in[4];
    int32_t h[4], w[4];
} gyre_fuser_input;

/* ControlNet (reference gyre/pipeline/controlnet/models.py ControlNetModel): the encoder-relevant fields of gyre_unet_cfg, the channels
 * of the hint image and the widths of its conditioning embedding. */
typedef struct {
    int32_t in_channels;             /* 4 */
    int32_t n_levels;                /* 4 */
    int32_t block_out_channels[GYRE_MAX_LEVELS]; /* 320,640,1280,1280 */
    int32_t layers_per_block;        /* 2 */
    int32_t attn_levels[GYRE_MAX_LEVELS];        /* 1,1,1,0 */
    int32_t num_heads[GYRE_MAX_LEVELS];          /* 8,8,8,8 */
    int32_t transformer_depth[GYRE_MAX_LEVELS];  /* 1,1,1,1 */
    int32_t cross_attention_dim;     /* 768 */
    int32_t norm_num_groups;         /* 32 */
    int32_t use_linear_projection;   /* 0 for SD1.x */
    int32_t flip_sin_to_cos;         /* 1 */
    float   freq_shift;              /* 0 */
    int32_t cond_channels;           /* 3: channels of the hint image */
    int32_t cond_embed_channels[4];  /* 16,32,96,256 (multiples of 8) */
} gyre_ctrl_cfg;

/* RRDBNet upscaler (BasicSR basicsr/archs/rrdbnet_arch.py RRDBNet; plus = 1: the reference's ResidualDenseBlock_Plus,
 * gyre/pipeline/upscalers/models/esrgan_plus.py) */
typedef struct {
    int32_t num_in_ch;               /* 3 */
    int32_t num_out_ch;              /* 3 */
    int32_t num_feat;                /* 64 (the only width built) */
    int32_t num_block;               /* 23 (esrgan, realesrgan-x4plus), 6 (realesrgan-x4plus-anime) */
    int32_t num_grow_ch;             /* 32 (the only width built) */
    int32_t scale;                   /* 4, 2 (pixel-unshuffle by 2 in front) or 1 (by 4) */
    int32_t plus;                    /* 1 = every dense block carries conv1x1 (ESRGAN+) */
} gyre_rrdb_cfg;

/* Epilogue of the dense-block convolution kernels, fp32, in this order, one rounding to storage:
 *   v = alpha * (acc + bias[n]);  if act: v = v > 0 ? v : 0.2f * v;  v += beta1 * r1[pix][n];  v += beta2 * r2[pix][n]
 * bias: [N_live] floats or NULL.  r1 / r2: first element of an NHWC storage slice with its own pixel stride (elements), or NULL; r1
 * may alias the output slice element for element. */
typedef struct {
    const float* bias; float alpha; int32_t act;
    const void* r1; int32_t ldr1; float beta1;
    const void* r2; int32_t ldr2; float beta2;
} gyre_rdb_epilogue;
/* One launch of the dense-block convolution: 3x3, stride 1, zero padding 1 over the first Cin channels of x (NHWC storage
 * [B][H][W], pixel stride ldx; ups = 1: nearest 2x inside the gather, output 2H x 2W), weights w [w_rows][9][Cin] in the library's
 * conv layout (w_rows <= NT; rows up to NT count as zero), the first N_live output channels written to out[pix][c0 .. c0 + N_live)
 * of a buffer with pixel stride ldo.  wpack: wpack_bytes >= NT * 9 * Cin * 2 bytes of scratch for the kernel's weight order. */
typedef struct {
    const void* x; int32_t ldx, Cin, B, H, W, ups;
    const void* w; int32_t w_rows, NT, N_live;
    void* out; int32_t c0, ldo;
    const gyre_rdb_epilogue* epi;
    void* wpack; size_t wpack_bytes;
} gyre_rdb_conv_args;

/* SwinIR upscaler (the reference's gyre/pipeline/upscalers/models/network_swinir.py, upsampler "nearest+conv").  Built: window 8,
 * embed_dim = 30 * heads with the same head count (<= 8) in every layer, mlp_hidden % 8 == 0, upscale 2 or 4, in_chans 3. */
typedef struct {
    int32_t in_chans;                /* 3 */
    int32_t embed_dim;               /* 180 (swinir), 240 (swinir-l) */
    int32_t num_layers;              /* RSTBs: 6 / 9 (<= 16) */
    int32_t depths[16];              /* blocks per RSTB: 6 */
    int32_t num_heads[16];           /* 6 / 8 */
    int32_t window_size;             /* 8 (the only one built) */
    int32_t mlp_hidden;              /* int(embed_dim * mlp_ratio): 360 / 480 */
    int32_t upscale;                 /* 4 or 2 */
    float img_range;                 /* 1.0 */
    int32_t resi_3conv;              /* 0 = "1conv", 1 = "3conv" */
} gyre_swinir_cfg;

/* HAT upscaler (the reference's gyre/pipeline/upscalers/models/hat_arch.py, upsampler "pixelshuffle", resi_connection "1conv").  Built:
 * window 16, overlap_ratio 0.5, compress_ratio 3, squeeze_factor 30, embed_dim = 30 * heads with the same head count (<= 8) in every
 * layer, mlp_hidden % 8 == 0, upscale 2 or 4, in_chans 3. */
typedef struct {
    int32_t in_chans;                /* 3 */
    int32_t embed_dim;               /* 180 */
    int32_t num_layers;              /* RHAGs: 6 (hat) / 12 (hat-l) (<= 16) */
    int32_t depths[16];              /* HABs per RHAG: 6 */
    int32_t num_heads[16];           /* 6 */
    int32_t window_size;             /* 16 (the only one built) */
    int32_t mlp_hidden;              /* int(embed_dim * mlp_ratio): 360 */
    int32_t upscale;                 /* 4 or 2 */
    float img_range;                 /* 1.0 */
    int32_t compress_ratio;          /* 3 */
    int32_t squeeze_factor;          /* 30 */
    float conv_scale;                /* 0.01 */
    float overlap_ratio;             /* 0.5 */
} gyre_hat_cfg;

/* Line-art hinter (the reference's gyre/pipeline/hinters/models/informative_drawings.py, DrawingGenerator; its three engines
 * hinters-lineart-anime / -contour / -opensketch are all input_nc 3, output_nc 1, n_residual_blocks 3).  Built: input_nc 3,
 * output_nc 1, 1 to 16 residual blocks, sigmoid 0 or 1. */
typedef struct {
    int32_t input_nc;                /* 3 */
    int32_t output_nc;               /* 1 */
    int32_t n_residual_blocks;       /* 3 as shipped, 9 the constructor's default (1 .. 16) */
    int32_t sigmoid;                 /* 1: the closing nn.Sigmoid */
} gyre_lineart_cfg;

/* One launch of the instance-normalisation apply pass (kernels_inorm.hip), for tests: out = relu?((x - mean) * rstd) (+ res) over the
 * logical image [B][H][W][C].  shuffled: x is [B][H/2][W/2][(a, b, C)] (a sub-pixel transposed convolution's output); res: the same
 * logical image stored with a border of res_pad pixels; pad 0 / 1 / 3: out is [B][H + 2 pad][W + 2 pad][C] with a mirrored border;
 * patch: out is [B][H][W][4 C], the 2x2 patch (y + dy, x + dx) in (dy, dx, c) order with zeros past the last row / column. */
typedef struct {
    const void* x; const float* stats; const void* res; void* out;
    int32_t B, H, W, C;
    int32_t shuffled, relu, res_pad, pad, patch;
} gyre_inorm_apply_args;

/* HED edge detector (the reference's gyre/pipeline/hinters/models/hed.py, HED; its engines hinters-hed / hinters-hed-alt).  The network
 * has no constructor arguments. */
typedef struct {
    int32_t reserved;                /* 0 */
} gyre_hed_cfg;

/* One launch of the HED fuse kernel (kernels_hed.hip), for tests: out [6][B][1][H][W] of out_dtype = sigmoid of so1 .. so5 (cropped) and
 * of their fuse.  so[k]: fp32 [B][Hk[k]][Wk[k]]; so[0] is read at (y + oy[0], x + ox[0]), so[k] (k = 1 .. 4) through its bilinear
 * transposed convolution of kernel 2 s, stride s = 1 << k, whose (Hk[k] + 1) s image is read at (y + oy[k], x + ox[k]); wf [5], bf [1]:
 * score_final. */
typedef struct {
    const float* so[5];
    int32_t Hk[5], Wk[5], oy[5], ox[5];
    const float* wf; const float* bf;
    void* out; int32_t out_dtype;
    int32_t B, H, W;
} gyre_hed_fuse_args;

/* MLSD line detector (the reference's gyre/pipeline/hinters/models/mbv2_mlsd_large.py, MobileV2_MLSD_Large).  The network has no
 * constructor arguments. */
typedef struct {
    int32_t reserved;                /* 0 */
} gyre_mlsd_cfg;

/* One launch of the BatchNorm fold (kernels_mlsd.hip), for tests: out = storage(w gamma / sqrt(var + 1e-5)), bias = beta + (conv_bias -
 * mean) gamma / sqrt(var + 1e-5) in fp32.  w: the PyTorch weight [O][I][k][k] as fp32 (kind 1, depthwise: [O][1][3][3]); conv_bias may
 * be null.  kind 0: out [o_pad][taps][i_pad], taps 1 or 9; kind 1: out [9][o_pad]; kind 2 (the entry convolution): out [9][I][o_pad].
 * bias [o_pad]; padding entries are zero. */
typedef struct {
    const float* w; const float* conv_bias; const float* gamma; const float* beta; const float* mean; const float* var;
    void* out; float* bias;
    int32_t kind, O, I, taps, o_pad, i_pad;
} gyre_mlsd_fold_args;

typedef struct gyre_unet gyre_unet;
typedef struct gyre_hed gyre_hed;
typedef struct gyre_mlsd gyre_mlsd;
typedef struct gyre_swinir gyre_swinir;
typedef struct gyre_hat gyre_hat;
typedef struct gyre_lineart gyre_lineart;
typedef struct gyre_vae gyre_vae;
typedef struct gyre_t2i gyre_t2i;
typedef struct gyre_t2i_seq gyre_t2i_seq;
typedef struct gyre_ctrl gyre_ctrl;
typedef struct gyre_rrdb gyre_rrdb;

/* ---- library ---------------------------------------------------------- */
int gyre_abi_version(void);
/* The 16-bit type this build stores activations and weights in (accumulation and all epilogues are fp32 in both): GYRE_BF16 for
 * libgyre_hip.so, GYRE_F16 for libgyre_hip_f16.so - the same sources and the same ABI built with -DGYRE_STORE_F16, the reference's own
 * GPU arithmetic (gyre/manager.py:146-151,1199-1200 loads its pipelines in fp16).  A caller picks the library by the torch_dtype
 * it loads the model in (gyre_amd/_lib.py lib(storage)); boundary tensors keep their per-call gyre_dtype in both. */
int gyre_storage_dtype(void);
const char* gyre_last_error(void);
/* number of distinct kernel launches issued by this thread's last forward/encode/decode */
int64_t gyre_last_launch_count(void);

/* ---- UNet --------------------------------------------------------------- */
int gyre_unet_create(const gyre_unet_cfg* cfg, int device, gyre_unet** out);
void gyre_unet_destroy(gyre_unet* h);
/* Number of parameter tensors the handle expects / key of the i-th one (diffusers name). */
int gyre_unet_num_params(const gyre_unet* h);
const char* gyre_unet_param_key(const gyre_unet* h, int i);
/* Copy+repack one tensor (PyTorch layout: conv OIHW, linear [out,in], vectors [n]) from
 * `dev_ptr` (contiguous, `dtype`) into library-owned bf16/f32 buffers.  Asynchronous on `stream`;
 * the source may be released once the stream has passed this point. */
int gyre_unet_set_weight(gyre_unet* h, const char* diffusers_key, const void* dev_ptr, int dtype,
                         const int64_t* shape, int ndim, void* stream);
/* Per-request LoRA without leaving the device.  The reference hooks  up(down(input)) * alpha / r * scale  onto every targeted
 * layer for one request and strips the hooks at the next (gyre/pipeline/lora.py:96-160); here the same linear map joins the
 * repack of the ONE weight it touches:
 *   packed(key) = round( k * ( base + sum_j scale_j * up_j down_j ) ),  summed in fp32, one rounding (k: the factor the library
 *   folds into some weights itself, e.g. the softmax scale in to_k)
 * base: the unpatched weight in PyTorch layout, as for gyre_unet_set_weight (same key and shape rules, GYRE_ERR_KEY);
 * up_j [O][rank] (x 1 x 1), down_j [rank][I] (x KH x KW), contiguous device tensors of pairs[j].dtype (GYRE_F32 / BF16 / F16, each
 * pair its own), rank >= 1, at most 8 pairs; scale_j = user scale * alpha / rank.  n_pairs == 0 writes exactly what
 * gyre_unet_set_weight writes: that takes a LoRA off again.  Vector keys (biases, norms), more than 8 pairs or rank < 1:
 * GYRE_ERR_INVALID.  Nothing else is uploaded: a finalized handle stays finalized (the key had been set before), the cached text
 * contexts are dropped, and the copies the library derives from weights (transposed, LayerNorm-folded, blocked, fragment-ordered,
 * folded-shortcut) are refreshed on the device by the next forward - all of them, they share one version counter.
 * Asynchronous on `stream`; base and the factors may be released once the stream has passed this point.
 * This entry is gyre_unet_set_weight_delta (below) restricted to GYRE_DELTA_LORA terms: pair j is the term (up_j, down_j, dtype,
 * rank, scale_j), the same kernel writes the same bits either way. */
typedef struct { const void* up; const void* down; int dtype; int rank; float scale; } gyre_lora_pair;
int gyre_unet_set_weight_lora(gyre_unet* h, const char* diffusers_key, const void* base, int base_dtype,
                              const int64_t* shape, int ndim, int n_pairs, const gyre_lora_pair* pairs, void* stream);
/* Per-request LyCORIS (LoCon, LoHa, LoKr, full diff) the same way.  The reference rebuilds  weight + sum updown  per targeted module
 * (gyre/pipeline/lycoris.py:99-228, 267-285); here each such delta is one TERM of the repack of the weight it touches:
 *   packed(key) = round( k * ( base + sum_j scale_j * D_j ) ),  summed in fp32 in term order, one rounding
 *   GYRE_DELTA_LORA  D = up[0] down[0]                                  up [O][rank] (x 1 x 1), down [rank][I] (x KH x KW)
 *   GYRE_DELTA_HADA  D = (up[0] down[0]) * (up[1] down[1]) element-wise, each pair with its own rank and dtype
 *   GYRE_DELTA_KRON  D[o1 O2 + o2][i1 I2 + i2](ky, kx) = w1[o1][i1] * W2[o2][i2](ky, kx),  w1 dense fp32 [O1][I1] with O1 | O, I1 | I;
 *                    W2 = up[0] [O2][rank] times down[0] [rank][I2] (x KH x KW), or with rank[0] == 0 the dense tensor down[0]
 *                    [O2][I2] (x KH x KW) (up[0] unused)
 *   GYRE_DELTA_FULL  D = down[0], a dense [O][I] (x KH x KW) tensor
 * Operands are contiguous device tensors of dtype[q] (GYRE_F32 / BF16 / F16) per (up, down) pair q.  A Tucker core is folded into the
 * right operand beforehand with gyre_op_lyco_core.  Same key and shape rules, version counter and finalize behaviour as
 * gyre_unet_set_weight_lora; 0 to 8 terms, n_terms == 0 writes gyre_unet_set_weight's bits.  GYRE_ERR_INVALID for vector keys,
 * a null operand, rank < 1 where a rank is needed, and Kronecker factors whose sizes do not multiply to the weight's; every
 * check precedes the launch and a refused call writes nothing. */
enum { GYRE_DELTA_LORA = 0, GYRE_DELTA_HADA = 1, GYRE_DELTA_KRON = 2, GYRE_DELTA_FULL = 3 };
typedef struct {
    int kind;
    const void* up[2]; const void* down[2]; int dtype[2]; int rank[2];
    const float* w1; int O1, I1;
    float scale;
} gyre_delta_term;
int gyre_unet_set_weight_delta(gyre_unet* h, const char* diffusers_key, const void* base, int base_dtype,
                               const int64_t* shape, int ndim, int n_terms, const gyre_delta_term* terms, void* stream);
/* 0 when every expected key has been set; otherwise GYRE_ERR_INCOMPLETE (message lists a missing key). */
int gyre_unet_finalize(gyre_unet* h, void* stream);
size_t gyre_unet_workspace_bytes(gyre_unet* h, int B, int H, int W, int S);
/* eps[B,out_ch,H,W] = unet(x[B,in_ch,H,W], t[B] (int64, dev), ctx[B,S,cross_dim]).
 * H, W are latent sizes and must be multiples of 2^(n_levels-1). */
int gyre_unet_forward(gyre_unet* h, void* stream,
                      const void* x_nchw, int x_dtype,
                      const int64_t* t_dev,
                      const void* ctx, int ctx_dtype,
                      int B, int H, int W, int S,
                      void* workspace, size_t workspace_bytes,
                      void* eps_out_nchw, int out_dtype);

/* Hint for the NEXT gyre_unet_forward* call on this handle only: all B entries of t_dev hold the same value (the samplers
 * of the reference pass ONE timestep per call: common_scheduler.py:344 / k-diffusion's sigma_to_t).  The time-embedding MLP and
 * the batched time_emb_proj then run for one row that every resnet reads - 1/B of that work, bit-identical results.  Ignored
 * when per-sample added conditioning (temb_add) is given.  A wrong hint gives every sample the first sample's timestep. */
int gyre_unet_hint_uniform_timestep(gyre_unet* h, int on);
/* (Both hints are the caller's word.  With GYRE_VERIFY_HINTS=1 in the environment every hinted call first checks the hint on the
 * device - one compare kernel over t / over the two halves of x, one 4-byte read-back, i.e. a stream synchronisation - and returns
 * GYRE_ERR_INVALID with a message instead of computing on a wrong assumption: the switch for bringing up a foreign caller.) */
/* Hint for the NEXT gyre_unet_forward* call on this handle only: the batch is a CFG-parallel pair batch as the reference builds
 * it (unet/cfg.py:49-57: latents cat[x, x], timesteps cat[t, t], contexts cat[uncond, cond]) - sample b and sample b + B/2 have
 * IDENTICAL latents and timestep and differ in their text context only.  Everything in front of the first cross-attention
 * (conv_in, the first resnet, the first transformer's GroupNorm / proj_in / self-attention: ~4 % of the FLOPs of an SD1.x call
 * at 64x64) is then evaluated once per pair and written twice: the two halves of a pair are IDENTICAL in that prefix, and equal
 * to the unshared call up to bf16 summation order (the prefix is planned for B/2 samples, so its tile / split-K choice - and with
 * it the order of the GroupNorm sums - may differ from the full batch's) - bit for bit under gyre_set_batch_invariant.  Ignored for odd B,
 * with ControlNet / T2I inputs, per-sample added conditioning or pending debug taps.  A wrong hint gives the second half of the
 * batch the first half's activations in that prefix. */
int gyre_unet_hint_cfg_pairs(gyre_unet* h, int on);

/* Text-context cache.  The context is constant over the 50+ UNet evaluations of a request, so its cross-attention
 * K / V projections (32 small GEMMs per call for SD1.x) can be done once: set_context projects ctx[B,S,cross_dim]
 * through every attn2.to_k / to_v into handle-owned buffers (may (re)allocate: not for the per-step path); afterwards
 * gyre_unet_forward / _ex accept ctx == NULL with the same B and S and reuse them.  Any set_weight invalidates it.
 * In the reference the same tensor is re-projected on every call (unet/core.py:253-259 binds it per wrapper). */
int gyre_unet_set_context(gyre_unet* h, void* stream, const void* ctx, int ctx_dtype, int B, int S);
/* The cache holds GYRE_CTX_SLOTS entries: the leaves of a hires-fix / graft tree and CFGUNet_Sequential
 * (unet/cfg.py:27-38, unet/hires_fix.py:123-235) alternate between two to four contexts on EVERY step.  _slot projects into
 * the given entry and makes it current (gyre_unet_set_context = slot 0); gyre_unet_select_context makes an already projected
 * entry current without any device work (GYRE_ERR_INVALID when that entry is empty or was invalidated by a set_weight). */
#define GYRE_CTX_SLOTS 4
int gyre_unet_set_context_slot(gyre_unet* h, void* stream, const void* ctx, int ctx_dtype, int B, int S, int slot);
int gyre_unet_select_context(gyre_unet* h, int slot);

/* Token merging (ToMe) for the UNet's self-attentions - the reference's pipeline option "tome: <r>"
 * (gyre/pipeline/unified_pipeline.py:1580-1588 -> nonfree/tome_patcher.py:14-52, nonfree/tome_unet.py:138-182,243):
 * before each self-attention the r most redundant keys (even token positions, by cosine similarity to their best
 * odd-position match - bipartite soft matching) are averaged into that match, values follow, and the attention runs
 * against N - r keys; r is clipped to N / 2 per layer as ToMe does.  0 switches it off (default).  The matching
 * algorithm lives in the un-vendored facebookresearch/ToMe submodule; restated from the paper, parity unpinned. */
int gyre_unet_set_tome(gyre_unet* h, int r);
/* Circular ("tiling") convolutions: the reference's request option `tiling` (True / "x" / "y" / "xy") patches every Conv2d of the
 * UNet and the VAE so that the module's own padding wraps around the image instead of reading zeros
 * (gyre/pipeline/unified_pipeline.py:1671-1712) - seamless textures.  mode: 0 off, 1 along x, 2 along y, 3 both; sticky until
 * changed.  The wrapped gather exists in the 4-wave conv kernels only, so such requests run slower; the input-gradient calls
 * (CLIP guidance) refuse it (GYRE_ERR_UNSUPPORTED). */
int gyre_unet_set_tiling(gyre_unet* h, int mode);
int gyre_vae_set_tiling(gyre_vae* h, int mode);

/* gyre_unet_forward_ex plus ControlNet-style residual injection - the optional keyword arguments of the reference's UNet call,
 * unet/core.py:40-64 (`down_block_additional_residuals`, `mid_block_additional_residual`) with the semantics of the in-tree
 * patcher controlnet/unet_patcher.py:30-95: down_res[k] (NCHW, dev, res_dtype; one per skip connection in production order,
 * conv_in's output first - 12 for SD1.x) is added to the skip tensor the up path consumes, mid_res to the mid block's output.
 * n_down_res == 0 / mid_res == NULL switch either off.
 * adapter_states (T2I adapters, unet/core.py:212-216 `adapter_states=`; semantics of t2i_adapter/unet_patcher.py:21-86): one
 * NCHW tensor (res_dtype) per down level, added in place to the level's last hidden state - before its downsampler on the
 * cross-attention levels (skip connection, downsampler and everything downstream see it), after the level otherwise. */
int gyre_unet_forward_ctrl(gyre_unet* h, void* stream, const void* x_nchw, int x_dtype, const int64_t* t_dev,
                           const void* ctx, int ctx_dtype, int B, int H, int W, int S,
                           void* workspace, size_t workspace_bytes, void* eps_out_nchw, int out_dtype, const float* temb_add,
                           const void* const* down_res, int n_down_res, int res_dtype, const void* mid_res,
                           const void* const* adapter_states, int n_adapter_states);

/* Input gradient (vector-Jacobian product) of the noise prediction: one call runs the forward pass, writes
 * eps_out_nchw like gyre_unet_forward, and writes dx_out_nchw[B, in_channels, H, W] = (d eps / d x)^T d_eps.
 * Replaces what autograd does in the reference's CLIP-guided mode, gyre/pipeline/unet/clipguided.py:301-338
 * (`latents.requires_grad_()`, `unet(latents, t)`) + :420 (`torch.autograd.grad(loss, latents)`); weights and the
 * text context receive no gradient there.  ctx must be passed (the K/V cache is not used); temb_add as in
 * gyre_unet_forward_ex (may be NULL).  With token merging enabled (gyre_unet_set_tome) the sweep re-derives the matching and
 * applies the merge's adjoint to d K / d V; the matching indices themselves carry no gradient (as under autograd). */
size_t gyre_unet_vjp_workspace_bytes(gyre_unet* h, int B, int H, int W, int S);
int gyre_unet_vjp(gyre_unet* h, void* stream, const void* x_nchw, int x_dtype, const int64_t* t_dev,
                  const void* ctx, int ctx_dtype, int B, int H, int W, int S,
                  const void* d_eps_nchw, int d_eps_dtype, void* workspace, size_t workspace_bytes,
                  void* eps_out_nchw, int out_dtype, void* dx_out_nchw, int dx_dtype, const float* temb_add);

/* The same in two calls, for an autograd node: _begin runs the forward pass (eps_out as gyre_unet_forward) and keeps the
 * activations the adjoints need in `workspace` (gyre_unet_vjp_workspace_bytes; must stay untouched), _finish runs the reverse
 * sweep for a cotangent.  At most one pending pair per handle: any other call on the handle in between drops the state and
 * _finish then returns GYRE_ERR_INVALID.  gyre_unet_vjp_pending tells the caller beforehand (1 = the state of the last _begin is
 * still there, 0 = dropped: fall back to the one-shot gyre_unet_vjp), so that a real argument error of _finish is never
 * mistaken for a dropped state. */
int gyre_unet_vjp_pending(gyre_unet* h);
int gyre_unet_vjp_begin(gyre_unet* h, void* stream, const void* x_nchw, int x_dtype, const int64_t* t_dev,
                        const void* ctx, int ctx_dtype, int B, int H, int W, int S, void* workspace, size_t workspace_bytes,
                        void* eps_out_nchw, int out_dtype, const float* temb_add);
int gyre_unet_vjp_finish(gyre_unet* h, void* stream, const void* d_eps_nchw, int d_eps_dtype, void* dx_out_nchw, int dx_dtype);
/* _finish for samples [b0, b0 + nb) of the pending forward pass only: d_eps / dx_out hold nb samples.  The reference's guided mode
 * differentiates the conditional evaluation and needs the unconditional one of the same latents right after
 * (unet/clipguided.py:218-241): one activation-keeping pass over cat[uncond, cond] (batch 2B) + the reverse sweep of the
 * conditional half replaces a batch-B keeping pass and a batch-B plain pass (SD1.5 + ToMe, B = 8: 19.8 against 12.6 + 11.7 ms). */
int gyre_unet_vjp_finish_range(gyre_unet* h, void* stream, const void* d_eps_nchw, int d_eps_dtype, void* dx_out_nchw, int dx_dtype,
                               int b0, int nb);

/* Parity tests only: the next forward copies the named intermediate activation (f32, NCHW) into out.  Names follow
 * the oracle's taps: "down<i>" (end of down level i, after its downsampler), "mid", "up<i>" (end of up level i, after
 * its upsampler), and the NODES by their state-dict prefix: "conv_in", every "<block>.resnets.<j>", every
 * "<block>.attentions.<j>" (the Transformer2D's output, after proj_out and its residual), every "<block>.downsamplers.0" /
 * "<block>.upsamplers.0".  A name this UNet does not have is GYRE_ERR_INVALID here, a buffer too small for the tensor is
 * GYRE_ERR_INVALID in the forward.  The next forward is a gyre_unet_forward* call or the activation-keeping pass of
 * gyre_unet_vjp / gyre_unet_vjp_begin; taps are cleared by it.
 * A tapped gyre_unet_forward* call loses two fusions, whatever the names: proj_out runs as its own launch instead of inside the
 * last FF2 (one rounding more per Transformer2D), and the halves of a CFG pair do not share their prefix
 * (gyre_unet_hint_cfg_pairs is ignored).  The activation-keeping pass has neither fusion and runs the same launches tapped or not. */
int gyre_unet_debug_tap(gyre_unet* h, const char* name, float* out_nchw_f32, size_t out_bytes);
/* Same for the reverse sweep: the next one (gyre_unet_vjp_finish, gyre_unet_vjp_finish_range or the sweep of gyre_unet_vjp) copies
 * the COMPLETE gradient of the named node's output into out - for a tensor that is also a skip connection the sum of the up
 * path's and the down path's contributions, i.e. what the adjoint of the node that produced it receives; for "conv_in" what the
 * adjoint of conv_in receives.  Node names only (no level names).  With a sample range the buffer holds nb samples.  The sweep
 * runs the same launches tapped or not.  Gradient taps are cleared by that sweep; a gyre_unet_forward* call, which drops a
 * pending forward state, clears them too. */
int gyre_unet_debug_grad_tap(gyre_unet* h, const char* name, float* out_nchw_f32, size_t out_bytes);
/* The same two taps on a VAE handle (one implementation: the name table and the copy are shared with the UNet's).  Forward NODES by
 * their state-dict prefix: "encoder.conv_in", "encoder.down_blocks.<i>.resnets.<j>", "encoder.down_blocks.<i>.downsamplers.0",
 * "encoder.mid_block.resnets.0" / ".attentions.0" (the attention block's output, after proj_attn and its residual) / ".resnets.1",
 * "encoder.conv_out" (what quant_conv reads); "post_quant_conv", "decoder.conv_in", "decoder.mid_block.*",
 * "decoder.up_blocks.<i>.resnets.<j>", "decoder.up_blocks.<i>.upsamplers.0".  There are no level names.
 * Forward taps belong to the NEXT gyre_vae_encode or gyre_vae_decode call, whichever comes first: it writes the taps of its own
 * half and drops all of them when it returns, so an encoder name set before a decode (or a decoder name before an encode) is
 * accepted here, never written and gone afterwards.  gyre_vae_decode_vjp serves no forward tap and leaves them pending.
 * Gradient taps exist for the decoder's nodes only ("post_quant_conv" and "decoder.*"; an encoder name is GYRE_ERR_INVALID here):
 * the next gyre_vae_decode_vjp copies the COMPLETE gradient of the node's output, as its sweep holds it, and drops every gradient
 * tap when it returns - also when it refuses the call (a tiling request is GYRE_ERR_UNSUPPORTED) and has written none.
 * A buffer too small for the tensor is GYRE_ERR_INVALID in the call that would write it.  Nothing in the VAE is fused differently
 * for a tap: a tapped call runs the launches of an untapped one plus one copy per tap, and writes the same output bits. */
int gyre_vae_debug_tap(gyre_vae* h, const char* name, float* out_nchw_f32, size_t out_bytes);
int gyre_vae_debug_grad_tap(gyre_vae* h, const char* name, float* out_nchw_f32, size_t out_bytes);

/* Same, plus an optional additive term for the time embedding: temb_add[B, 4*block_out_channels[0]] (f32, dev) is
 * added to time_embedding(t) before it feeds the ResNet blocks.  This is how SDXL's `text_time` added conditioning
 * (add_embedding MLP over pooled text + size/crop ids, a few MFLOP) enters: the MLP stays host PyTorch. */
int gyre_unet_forward_ex(gyre_unet* h, void* stream, const void* x_nchw, int x_dtype, const int64_t* t_dev,
                         const void* ctx, int ctx_dtype, int B, int H, int W, int S,
                         void* workspace, size_t workspace_bytes, void* eps_out_nchw, int out_dtype,
                         const float* temb_add_dev);

/* ---- VAE ---------------------------------------------------------------- */
int gyre_vae_create(const gyre_vae_cfg* cfg, int device, gyre_vae** out);
void gyre_vae_destroy(gyre_vae* h);
int gyre_vae_num_params(const gyre_vae* h);
const char* gyre_vae_param_key(const gyre_vae* h, int i);
int gyre_vae_set_weight(gyre_vae* h, const char* diffusers_key, const void* dev_ptr, int dtype,
                        const int64_t* shape, int ndim, void* stream);
int gyre_vae_finalize(gyre_vae* h, void* stream);
size_t gyre_vae_workspace_bytes(gyre_vae* h, int B, int H, int W, int decode);
/* moments[B,2*z,H/8,W/8] (mean | logvar, f32) = quant_conv(encoder(image[B,3,H,W] in -1..1)) */
int gyre_vae_encode(gyre_vae* h, void* stream, const void* image_nchw, int in_dtype, int B, int H, int W,
                    void* workspace, size_t workspace_bytes, void* moments_out_nchw, int out_dtype);
/* image[B,3,8h,8w] = decoder(post_quant_conv(z[B,z,h,w])) */
int gyre_vae_decode(gyre_vae* h, void* stream, const void* z_nchw, int in_dtype, int B, int h_lat, int w_lat,
                    void* workspace, size_t workspace_bytes, void* image_out_nchw, int out_dtype);

/* ---- T2I adapter ------------------------------------------------------------ */
/* Weight keys are the state-dict keys of the reference's Adapter / Adapter_light.  Same weight store, workspace and dry-run sizing
 * rules as the UNet and the VAE. */
int gyre_t2i_create(const gyre_t2i_cfg* cfg, int device, gyre_t2i** out);
void gyre_t2i_destroy(gyre_t2i* h);
int gyre_t2i_num_params(const gyre_t2i* h);
const char* gyre_t2i_param_key(const gyre_t2i* h, int i);
int gyre_t2i_set_weight(gyre_t2i* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, void* stream);
int gyre_t2i_finalize(gyre_t2i* h, void* stream);
size_t gyre_t2i_workspace_bytes(gyre_t2i* h, int B, int H, int W);
/* features_out_nchw[i] [B, channels[i], H/8 >> i, W/8 >> i] = level i of the adapter over image[B, cin/64, H, W] (H, W multiples
 * of 8; n = n_levels).  The stride-2 conv downsampling (use_conv) rounds an odd size up, the average pool down, as torch does. */
int gyre_t2i_forward(gyre_t2i* h, void* stream, const void* image_nchw, int in_dtype, int B, int H, int W,
                     void* workspace, size_t workspace_bytes, void* const* features_out_nchw, int n, int out_dtype);

/* ---- T2I style adapter and co-adapter fuser --------------------------------- */
/* Weight keys are the state-dict keys of the reference's StyleAdapter / CoAdapterFuser (transformer_layes.{i}.attn.in_proj_weight, ...,
 * style_embedding, proj / task_embedding, positional_embedding, spatial_feat_mapping.{i}.1, spatial_ch_projs.{i}, seq_proj); proj and
 * seq_proj, used as x @ P, are stored transposed at load.  Same weight store, workspace and dry-run sizing rules as the other handles.
 * workspace_bytes: style - S input tokens (n_spatial ignored); fuser - S = the token rows of all token inputs together, n_spatial = the
 * number of spatial inputs.  A sequence longer than gyre_op_seq_attn_max_len(width / num_head) is GYRE_ERR_UNSUPPORTED (0 here). */
int gyre_t2i_seq_create(const gyre_t2i_seq_cfg* cfg, int device, gyre_t2i_seq** out);
void gyre_t2i_seq_destroy(gyre_t2i_seq* h);
int gyre_t2i_seq_num_params(const gyre_t2i_seq* h);
const char* gyre_t2i_seq_param_key(const gyre_t2i_seq* h, int i);
int gyre_t2i_seq_set_weight(gyre_t2i_seq* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, void* stream);
int gyre_t2i_seq_finalize(gyre_t2i_seq* h, void* stream);
size_t gyre_t2i_seq_workspace_bytes(gyre_t2i_seq* h, int N, int S, int n_spatial);
/* out[N][num_token][context_dim] = ln_post(blocks(ln_pre(cat[x, style_embedding]))[:, -num_token:]) @ proj over x[N][S][width]. */
int gyre_t2i_style_forward(gyre_t2i_seq* h, void* stream, const void* x, int in_dtype, int N, int S, void* workspace, size_t workspace_bytes,
                           void* out, int out_dtype);
/* CoAdapterFuser.forward over the inputs in their order.  maps_out[i] NCHW storage [N][unet_channels[i]][h[i]][w[i]] = the sum over the
 * spatial inputs of state (alpha + 1) (null when there is no spatial input); tokens_out [N][sum of T][width] of token_dtype = the
 * token inputs, each times (x @ seq_proj + 1), concatenated in order (null when there is no token input). */
int gyre_t2i_fuser_forward(gyre_t2i_seq* h, void* stream, const gyre_fuser_input* inputs, int n_inputs, int token_dtype, int N,
                           void* workspace, size_t workspace_bytes, void* const* maps_out, void* tokens_out);

/* ---- RRDBNet upscaler ------------------------------------------------------- */
/* Weight keys are BasicSR's state-dict names: conv_first, body.{i}.rdb{1,2,3}.conv{1..5}.{weight,bias}, body.{i}.rdb{j}.conv1x1.weight
 * (plus), conv_body, conv_up1, conv_up2, conv_hr, conv_last.  Same weight store, workspace and dry-run sizing rules as the other
 * handles.  num_feat != 64 or num_grow_ch != 32: GYRE_ERR_UNSUPPORTED at create. */
int gyre_rrdb_create(const gyre_rrdb_cfg* cfg, int device, gyre_rrdb** out);
void gyre_rrdb_destroy(gyre_rrdb* h);
int gyre_rrdb_num_params(const gyre_rrdb* h);
const char* gyre_rrdb_param_key(const gyre_rrdb* h, int i);
int gyre_rrdb_set_weight(gyre_rrdb* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, void* stream);
int gyre_rrdb_finalize(gyre_rrdb* h, void* stream);
size_t gyre_rrdb_workspace_bytes(gyre_rrdb* h, int B, int H, int W);
/* out[B, num_out_ch, H * scale, W * scale] = RRDBNet(image[B, num_in_ch, H, W]).  H and W must be multiples of 2 / 4 for scale
 * 2 / 1 (GYRE_ERR_INVALID otherwise).  A sample's result does not depend on the batch it runs in. */
int gyre_rrdb_forward(gyre_rrdb* h, void* stream, const void* image_nchw, int in_dtype, int B, int H, int W,
                      void* workspace, size_t workspace_bytes, void* out_nchw, int out_dtype);
/* Which kernel the 3x3 convolutions take: 0 auto (the fused dense-block kernel where it measured faster), 1 generic (the planner's
 * GEMM kernels with bias only, then the epilogue kernel in place), 2 fused everywhere; tuning: 0x100 | mask takes the fused kernel for
 * exactly the shape groups of the mask (bit 0 conv1-4 of a dense block, 1 conv5, 2 the upsampling convolutions, 3 conv_last,
 * 4 conv_first / conv_body / conv_hr).  The workspace size depends on the path. */
int gyre_rrdb_set_path(gyre_rrdb* h, int path);

/* ---- SwinIR upscaler -------------------------------------------------------- */
/* Weight keys are the reference's state-dict names: conv_first, patch_embed.norm, layers.{i}.residual_group.blocks.{j}.{norm1,
 * attn.relative_position_bias_table, attn.qkv, attn.proj, norm2, mlp.fc1, mlp.fc2}, layers.{i}.conv (3conv: .conv.0 / .2 / .4), norm,
 * conv_after_body (3conv: .0 / .2 / .4), conv_before_upsample.0, conv_up1, conv_up2 (x4 only), conv_hr, conv_last.  Same weight store,
 * workspace and dry-run sizing rules as the other handles.  A configuration outside the built list (gyre_swinir_cfg): GYRE_ERR_UNSUPPORTED
 * at create. */
int gyre_swinir_create(const gyre_swinir_cfg* cfg, int device, gyre_swinir** out);
void gyre_swinir_destroy(gyre_swinir* h);
int gyre_swinir_num_params(const gyre_swinir* h);
const char* gyre_swinir_param_key(const gyre_swinir* h, int i);
int gyre_swinir_set_weight(gyre_swinir* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, void* stream);
int gyre_swinir_finalize(gyre_swinir* h, void* stream);
size_t gyre_swinir_workspace_bytes(gyre_swinir* h, int B, int H, int W);
/* out[B, 3, H * upscale, W * upscale] = SwinIR(image[B, 3, H, W]).  H and W must be multiples of 8 (GYRE_ERR_INVALID otherwise; the
 * reflect padding of check_image_size is the caller's).  Blocks with an odd index use the shift 4, except on an image of one window per
 * side.  A sample's result does not depend on the batch it runs in. */
int gyre_swinir_forward(gyre_swinir* h, void* stream, const void* image_nchw, int in_dtype, int B, int H, int W,
                        void* workspace, size_t workspace_bytes, void* out_nchw, int out_dtype);

/* ---- HAT upscaler ----------------------------------------------------------- */
/* Weight keys are the reference's state-dict names: conv_first, patch_embed.norm, layers.{i}.residual_group.blocks.{j}.{norm1,
 * attn.relative_position_bias_table, attn.qkv, attn.proj, conv_block.cab.0, conv_block.cab.2, conv_block.cab.3.attention.1,
 * conv_block.cab.3.attention.3, norm2, mlp.fc1, mlp.fc2}, layers.{i}.residual_group.overlap_attn.{norm1, qkv,
 * relative_position_bias_table, proj, norm2, mlp.fc1, mlp.fc2}, layers.{i}.conv, norm, conv_after_body, conv_before_upsample.0,
 * upsample.0, upsample.2 (x4 only), conv_last.  Same weight store, workspace and dry-run sizing rules as the other handles.  A
 * configuration outside the built list (gyre_hat_cfg): GYRE_ERR_UNSUPPORTED at create. */
int gyre_hat_create(const gyre_hat_cfg* cfg, int device, gyre_hat** out);
void gyre_hat_destroy(gyre_hat* h);
int gyre_hat_num_params(const gyre_hat* h);
const char* gyre_hat_param_key(const gyre_hat* h, int i);
int gyre_hat_set_weight(gyre_hat* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, void* stream);
int gyre_hat_finalize(gyre_hat* h, void* stream);
size_t gyre_hat_workspace_bytes(gyre_hat* h, int B, int H, int W);
/* out[B, 3, H * upscale, W * upscale] = HAT(image[B, 3, H, W]).  H and W must be positive multiples of 16 (GYRE_ERR_INVALID otherwise:
 * the reference has no padding either).  HABs with an odd index use the shift 8, also on an image of one window per side.  A sample's
 * result does not depend on the batch it runs in. */
int gyre_hat_forward(gyre_hat* h, void* stream, const void* image_nchw, int in_dtype, int B, int H, int W,
                     void* workspace, size_t workspace_bytes, void* out_nchw, int out_dtype);

/* ---- line-art hinter -------------------------------------------------------
 * Replaces the host model behind the reference's edge_detection task for the informative-drawings engines (services/generate.py:315-317).
 * Weight keys, in the reference's state-dict order (.weight and .bias each): model0.1, model1.0, model1.3, model2.{i}.conv_block.1,
 * model2.{i}.conv_block.5, model3.0, model3.3 (ConvTranspose2d layout [Cin, Cout, 3, 3]), model4.1.  The instance normalisations are
 * affine-free and have no keys.  Same weight store, workspace and dry-run sizing rules as the other handles.  A configuration outside
 * the built list (gyre_lineart_cfg): GYRE_ERR_UNSUPPORTED at create. */
int gyre_lineart_create(const gyre_lineart_cfg* cfg, int device, gyre_lineart** out);
void gyre_lineart_destroy(gyre_lineart* h);
int gyre_lineart_num_params(const gyre_lineart* h);
const char* gyre_lineart_param_key(const gyre_lineart* h, int i);
int gyre_lineart_set_weight(gyre_lineart* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, void* stream);
int gyre_lineart_finalize(gyre_lineart* h, void* stream);
size_t gyre_lineart_workspace_bytes(gyre_lineart* h, int B, int H, int W);
/* out[B, 1, Ho, Wo] = DrawingGenerator(image[B, 3, H, W]) with Ho = 4 ceil(ceil(H / 2) / 2) (= H when H % 4 == 0; W alike), the size
 * the reference's layers produce.  H, W >= 5 (GYRE_ERR_INVALID below: torch's reflection paddings refuse those too).  A sample's
 * result does not depend on the batch it runs in. */
int gyre_lineart_forward(gyre_lineart* h, void* stream, const void* image_nchw, int in_dtype, int B, int H, int W,
                         void* workspace, size_t workspace_bytes, void* out_nchw, int out_dtype);

/* ---- HED edge detector -----------------------------------------------------
 * Replaces the host model behind the reference's edge_detection task for the hinters-hed engines.  Weight keys, in the reference's
 * state-dict order (.weight and .bias each): conv1_1, conv1_2, conv2_1, conv2_2, conv3_1 .. conv3_3, conv4_1 .. conv4_3, conv5_1 ..
 * conv5_3, score_dsn1 .. score_dsn5, score_final (38 entries; the bilinear weight_deconv buffers are not persistent and have no keys).
 * Same weight store, workspace and dry-run sizing rules as the other handles. */
int gyre_hed_create(const gyre_hed_cfg* cfg, int device, gyre_hed** out);
void gyre_hed_destroy(gyre_hed* h);
int gyre_hed_num_params(const gyre_hed* h);
const char* gyre_hed_param_key(const gyre_hed* h, int i);
int gyre_hed_set_weight(gyre_hed* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, void* stream);
int gyre_hed_finalize(gyre_hed* h, void* stream);
size_t gyre_hed_workspace_bytes(gyre_hed* h, int B, int H, int W);
/* out[6][B][1][H][W] = HED(image[B, 3, H, W]): the five side outputs and their fuse, each already sigmoided, in the reference's order.
 * H, W >= 1; B (H + 68)(W + 68) < 2^30 (GYRE_ERR_INVALID otherwise, before any launch).  A sample's result does not depend on the batch
 * it runs in. */
int gyre_hed_forward(gyre_hed* h, void* stream, const void* image_nchw, int in_dtype, int B, int H, int W,
                     void* workspace, size_t workspace_bytes, void* out, int out_dtype);
/* The geometry of an image side n: sizes[5] = n + 68 and its ceil halves, offsets[5] = the crop offsets int(round(d / 2.)) of the five
 * maps, halves to even as Python rounds. */
int gyre_hed_geometry(int n, int32_t* sizes, int32_t* offsets);

/* ---- MLSD line detector ----------------------------------------------------
 * The reference vendors the network (MobileV2_MLSD_Large) whose output the straight-line hint of the controlnet/mlsd hintsets is decoded
 * from.  Weight keys, in the reference's state-dict order: backbone.features.0.{0.weight, 1.*}, backbone.features.1 .. 13.conv.*,
 * block15 .. block22.{conv1, conv2}.{0.weight, 0.bias, 1.*}, block23.{conv1, conv2}.*, block23.conv3.{weight, bias}, where 1.* of a
 * BatchNorm is weight, bias, running_mean, running_var: 305 entries, the reference's 362 less the 57 num_batches_tracked counters,
 * which are not keys.  set_weight stages the raw parameters in fp32; finalize folds every BatchNorm (eval mode, eps 1e-5) into its
 * convolution in fp32 and rounds the result once to storage.  Same workspace and dry-run sizing rules as the other handles. */
int gyre_mlsd_create(const gyre_mlsd_cfg* cfg, int device, gyre_mlsd** out);
void gyre_mlsd_destroy(gyre_mlsd* h);
int gyre_mlsd_num_params(const gyre_mlsd* h);
const char* gyre_mlsd_param_key(const gyre_mlsd* h, int i);
int gyre_mlsd_set_weight(gyre_mlsd* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, void* stream);
int gyre_mlsd_finalize(gyre_mlsd* h, void* stream);
size_t gyre_mlsd_workspace_bytes(gyre_mlsd* h, int B, int H, int W);
/* out[B][9][H / 2][W / 2] = MobileV2_MLSD_Large(image[B, 4, H, W]), channels 7 .. 15 of the network's 16-channel map.  H and W: at least
 * 16 with (H / 2) % 8 == 0, the sizes at which the reference's concatenations line up (GYRE_ERR_INVALID otherwise, before any launch).
 * A sample's result does not depend on the batch it runs in. */
int gyre_mlsd_forward(gyre_mlsd* h, void* stream, const void* image_nchw, int in_dtype, int B, int H, int W,
                      void* workspace, size_t workspace_bytes, void* out_nchw, int out_dtype);

/* ---- ControlNet ------------------------------------------------------------ */
/* Weight keys are the diffusers ControlNetModel state-dict keys: conv_in, time_embedding.*, down_blocks.*, mid_block.* as in the UNet,
 * controlnet_cond_embedding.{conv_in, blocks.0..5, conv_out}, controlnet_down_blocks.0..N-1 and controlnet_mid_block, with
 * N = 1 + n_levels * layers_per_block + (n_levels - 1) skip connections (12 for SD1.x).  Same weight store, workspace and dry-run
 * sizing rules as the UNet.  The model runs in two parts:
 *   bind, once per request: the conditioning embedding of image[image_B, cond_channels, image_H, image_W] (image_H, image_W
 *     multiples of 8; image_B == B, or 1: the one image serves every sample) and the cross-attention K / V of context[B, S, D]
 *     through this model's own weights, both kept in buffers the handle owns (a set_weight call drops them);
 *   forward, once per step: x[B, in_channels, H, W] and t[B] -> N + 1 residuals, the k-th being scales[k] (host floats) times the zero
 *     convolution of the k-th skip connection (conv_in first), the last that of the mid block.  They go to samples
 *     [out_b0, out_b0 + B) of outs[k] [out_B, C_k, H_k, W_k] NCHW of out_dtype: accumulate == 0 assigns and writes every other
 *     sample of outs[k] as zero (the unconditional half of a cfg_only hint), accumulate == 1 adds (one fp32 add, one rounding) and
 *     leaves the other samples alone (the sum over several control models).
 * forward before bind, a batch other than the bound one, and an H x W other than the bound image's size / 8: GYRE_ERR_INVALID.
 *
 * Bind slots.  The handle keeps GYRE_CTRL_SLOTS independent binds: the leaves of a hires-fix / graft tree alternate on one control
 * model every step, each with its own hint image, context and size, and re-embedding the image per call would cost more than the
 * step.  gyre_ctrl_bind / gyre_ctrl_forward are slot 0, unmasked, and behave exactly as before.  A slot owns its conditioning
 * embedding, its projected K / V, its geometry (batch, image H x W, S) and, optionally, its residual masks: res_masks[k] (k < n_masks
 * == N + 1, device pointers) is fp32 [mask_B, 1, h_k, w_k] with mask_B == 1 or B and mask_hw[2k], mask_hw[2k + 1] == the size of
 * residual k; they are copied into buffers the handle owns during the bind.  res_masks == NULL or all entries NULL: unmasked.  With
 * masks residual k is  rnd(fl(fl(scales[k] r) m) [+ old])  - fp32 products, the accumulate add, one rounding to out_dtype; m == 0 gives
 * +-0 for a finite r, NaN stays NaN.
 * gyre_ctrl_forward_slot takes, optionally, x_mask fp32 [x_mask_B, 1, H, W] (x_mask_B == 1 or B; NULL: none): the entry pass
 * multiplies x[b, c, p] by x_mask[b or 0, 0, p] in fp32 from the source dtype with one rounding to storage (next to a 9-channel inpaint
 * UNet the reference feeds the control model latents[:, 0:4] * latents[:, [4]]).
 * gyre_ctrl_set_weight drops every slot.  GYRE_ERR_INVALID: forward on an unbound slot, a slot outside [0, GYRE_CTRL_SLOTS), a
 * geometry other than the slot's, masks that are partly NULL, and a mask whose size is not its residual's. */
#define GYRE_CTRL_SLOTS 4
int gyre_ctrl_create(const gyre_ctrl_cfg* cfg, int device, gyre_ctrl** out);
void gyre_ctrl_destroy(gyre_ctrl* h);
int gyre_ctrl_num_params(const gyre_ctrl* h);
const char* gyre_ctrl_param_key(const gyre_ctrl* h, int i);
int gyre_ctrl_set_weight(gyre_ctrl* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, void* stream);
int gyre_ctrl_finalize(gyre_ctrl* h, void* stream);
size_t gyre_ctrl_bind_workspace_bytes(gyre_ctrl* h, int image_B, int image_H, int image_W, int B);
int gyre_ctrl_bind(gyre_ctrl* h, void* stream, const void* image_nchw, int image_dtype, int image_B, int image_H, int image_W,
                   const void* context, int ctx_dtype, int B, int S, void* workspace, size_t workspace_bytes);
size_t gyre_ctrl_workspace_bytes(gyre_ctrl* h, int B, int H, int W, int S);
int gyre_ctrl_forward(gyre_ctrl* h, void* stream, const void* x_nchw, int x_dtype, const int64_t* t, int B, int H, int W,
                      void* workspace, size_t workspace_bytes, const float* scales, int accumulate, int out_B, int out_b0,
                      void* const* outs_nchw, int n_outs, int out_dtype);
size_t gyre_ctrl_bind_slot_workspace_bytes(gyre_ctrl* h, int slot, int image_B, int image_H, int image_W, int B);
int gyre_ctrl_bind_slot(gyre_ctrl* h, void* stream, int slot, const void* image_nchw, int image_dtype, int image_B, int image_H,
                        int image_W, const void* context, int ctx_dtype, int B, int S, const float* const* res_masks,
                        const int32_t* mask_hw, int n_masks, int mask_B, void* workspace, size_t workspace_bytes);
int gyre_ctrl_forward_slot(gyre_ctrl* h, void* stream, int slot, const void* x_nchw, int x_dtype, const float* x_mask, int x_mask_B,
                           const int64_t* t, int B, int H, int W, void* workspace, size_t workspace_bytes, const float* scales,
                           int accumulate, int out_B, int out_b0, void* const* outs_nchw, int n_outs, int out_dtype);

/* ---- per-launch timing with HIP events on the launch stream (bench.py roofline leg) ----
 * mask: bit k enables kernel class k (names from gyre_prof_class_name; they equal the prefix of the
 * kernel's demangled name as rocprofv3 prints it).  collect(): after the caller synchronised the
 * stream, returns per class the number of timed launches, the summed event-to-event milliseconds and
 * the summed ALGORITHMIC flops / bytes (unpadded problem sizes) and clears the records. */
int gyre_prof_set_mask(unsigned long long mask);
int gyre_prof_num_classes(void);
const char* gyre_prof_class_name(int kclass);
int gyre_prof_collect(int64_t* launches, double* ms, double* flops, double* bytes);

/* Tests / tuning only: force the GEMM tile configuration of this thread's following launches
 * (0 = automatic; 1 = 4-wave 128x128, 2 = 4-wave 256x64, 3 = 4-wave 64x64, 4 = 8-wave 256x320,
 * 5 = 8-wave 128x320, 6 = 8-wave 256x256, 7 = 8-wave 128x256 (8 = 128x160, 12 = 256x128 convolutions only, 20 - 24 pipelined forms,
 * 30 / 31 A- / W-resident, 32 small-problem kernel); bits 8-15 = split-K factor for the 8-wave
 * configs, 0/1 = none).  Returns the previous value. */
int gyre_debug_force_gemm_cfg(int cfg);
/* Tests / tuning only: split-K slab space for this thread's gyre_op_* calls (the model handles carve theirs from
 * the caller's workspace).  Without it the single operators run the best single-split configuration. */
int gyre_debug_set_splitk_workspace(void* ws_dev, size_t bytes);
/* Tests / tuning only: scratch space (N * K * 2 bytes) where this thread's gyre_op_* calls pack the weights for the A-resident
 * GEMM kernel (tile config 30: K = 320 / 640 linear problems; the model handles keep a packed copy per weight).  With it the
 * planner may choose that kernel for single operators; NULL / 0 = off. */
int gyre_debug_set_ar_workspace(void* ws_dev, size_t bytes);
/* Tests / tuning only: scratch space (N * K * 2 bytes) where this thread's gyre_op_* calls make the BLOCKED weight copy the LDS-DMA tile
 * kernels read for K > 1024 (1-KiB blocks of 8 rows x 64 k; the model handles keep one per weight).  NULL / 0 = off: row-major weights. */
int gyre_debug_set_wblk_workspace(void* ws_dev, size_t bytes);
/* Tests / tuning only: 0 automatic, 1 = register-staged attention kernel, 2 / 4 = LDS-DMA kernel with 32 / 64
 * query rows per wave; with prescaled K: 3 = folded-softmax v2 kernel, 5 = software-pipelined v3 kernel (head dims
 * 16/32/40/64); 6 = automatic without the several-query-blocks-per-workgroup form of short key sequences; 7 = automatic with the
 * pipelined kernel's per-tile overflow check in every tile (the round-3 kernel); 0 / 8 = automatic: head dims <= 40 run the optimistic
 * first pass (no per-tile check; a workgroup whose row sums leave (0, 2^60) repeats its pass with the check - since round 6 that
 * bound equals the checked pass's re-centring threshold, so the default is bit-identical to variant 7 on every input).  The round-4
 * non-reproducibility of that pass under concurrent handles was a ring-slot hazard, fixed in round 5 (kernels_attn.hip header).
 * Returns the previous value. */
int gyre_debug_force_attn_variant(int v);
/* The number of attention workgroups on the CURRENT device that have repeated their pass with the per-tile overflow check so far in
 * this process (always counted since round 6: the increment sits on the redo path only; one blocking 4-byte read-back per call;
 * -1: no device / allocation failure).  bench.py reports the count of its timed region as `attn_redo_count`. */
long gyre_debug_attn_redo_count(void);
/* What gyre_op_attention_ex / gyre_op_attention_bwd would launch for these sizes under the calling thread's forced variant, without
 * touching a device (tests/test_attn_plan_host.py).  Return value: the status the launch would give (message in gyre_last_error()).
 * gyre_debug_attn_plan: out[12] = kernel family (0 k_attn, 1 k_attn2 plain, 2 k_attn2 folded, 3 k_attn3), D, query fragments per wave
 * (QI), ring lookahead (PD), ring slots, dynamic LDS bytes, grid x / y / z, query blocks per workgroup (qiter), always_check, QLOOP.
 * gyre_debug_attn_bwd_plan: out[10] = family (0 LDS-DMA D = 40, 1 LDS-tile, 2 register-staged), the head-dim bound of the kernel
 * set's row, d-chunks, dynamic LDS bytes, dQ grid x / y / z, dK / dV grid x / y / z (zeros without with_dk).
 * gyre_debug_attn_tables: the kernel sets a launch can reach - which = 0: (family, D, QI, QLOOP) per forward row; 1 / 2: the bound of
 * every LDS-tile / register-staged backward row; at most cap ints are written, the number of rows is returned. */
int gyre_debug_attn_plan(int B, int H, int Nq, int Nk, int D, int k_prescaled, int ldq, int ldk, int ldvt, int ldo, int32_t* out);
int gyre_debug_attn_bwd_plan(int B, int H, int Nq, int Nk, int D, int with_dk, int32_t* out);
int gyre_debug_attn_tables(int which, int32_t* out, int cap);
/* Tuning only: per-workgroup cycle stamps of the fused cross-attention kernel's phase boundaries (8 x uint64 per workgroup of the
 * last launch) into a caller-allocated device buffer; NULL = off (tools/r06_xattn_phases.py). */
int gyre_debug_xattn_stamps(void* dev_buf);
/* Tuning only.  Ablations (results are garbage): bit0 = skip the operand loads inside the K loop, bit1 = skip the MFMAs,
 * bit2 = no epilogue.  Planner switches for same-box A/B runs (results stay valid): bit8 = default tile order, bit9 = conv
 * zero padding from a zero page in the pipelined kernel, bit10 = no pipelined (32x32x16) tile configs, bit11 = LayerNorm as a
 * separate pass (no fold into the consuming GEMM), bit15 = folded LayerNorm takes its row statistics from a separate pass
 * instead of the producing GEMM's epilogue, bit16 = the GEGLU FF1 keeps its separate LayerNorm, bit17 = GroupNorm keeps its own
 * statistics pass (no statistics from the producing conv / GEMM), bit19 = slab-outer GEGLU epilogue of the folded-LayerNorm
 * FF1, bit20 = no statistics epilogue on the 128x160 tile, bit21 = no A-resident kernel (K = 320 / 640 linear problems go to the
 * 8-wave tiles as before), bit22 = A-resident kernel also for the C x C projections (N < 3 K),
 * bit12 = the Transformer2D GroupNorm keeps its apply pass (no fold into proj_in), bit23 = no pipelined 256x320 tile
 * for 3x3 convs whose grid of it has 128 - 159 workgroups (the 48x48 level of a 768 px request), bit5 = no small-problem kernel
 * (tile config 32, kernels_gemm_sm.hip): small linear problems go to the register-staged 4-wave tiles as before, bit6 = it does not take
 * the long-K few-row linear problems from the split-K path.  Round 5: bit24 = the two-stage K loop in the 8-wave kernels' linear mode
 * (instead of the 2 - 4 stage LDS ring with counted waits), bit25 = the deep ring at one workgroup per CU also where two 2-stage
 * workgroups would fit, bit26 = row-major weights everywhere (no blocked weight copies for the LDS-DMA kernels), bit27 = the two-stage K loop for the
 * 128x160 tile's 3x3 convolutions (instead of the same ring).  Round 6: bit13 = no fused cross-attention kernel (kernels_xattn.hip:
 * to_q -> attention -> to_out of SD1.x's 64x64 level in one launch): the three-launch chain as before.  (Bit 7 - the small kernel's
 * LayerNorm fold - went with the code it switched on; the bit is reused:) bit7 = the 1x1 shortcut of a channel-changing / concat resnet
 * stays its own launch instead of riding inside conv2 as extra K steps of the pipelined tile (round 6).
 * Round 7: bit28 = a Transformer2D's proj_out stays its own launch instead of riding inside the FF2 of its last block as extra K
 * steps on composed weights.
 * Round 12: bit29 = the UNet upsampler convs keep nine taps (no four-parity 2x2 form on composed weights), bit30 = that form wherever
 * the kernel supports the shape, whatever the planner's tile-count rule (tile config 24 for that conv; tests and tuning on small shapes).
 * Epilogue ablations (garbage): bit3 = no GELU, bit4 = no stores.
 * These switches are PER CALLING THREAD (thread-local, like gyre_set_batch_invariant): they never change what another thread's
 * handle computes. */
int gyre_debug_gemm_ablation(int bits);
/* Shape query, no device: 1 when gyre_op_ln_linear keeps the folded form for this plain / GEGLU linear (N as there), else 0. */
int gyre_debug_ln_linear_folds(int M, int K, int N, int geglu);
/* Shape query, no device: 1 when gyre_op_groupnorm runs the one-launch two-pass kernel for this shape (C1 = C for one source). */
int gyre_debug_gn_uses_small(int HW, int C, int C1, int groups);
/* Tests / tuning only: one GEMM / implicit-GEMM 3x3 convolution launch described field by field, for the inputs the model runtime
 * produces and no gyre_op_* entry can express (tests/test_gpu_gemm_exact.py).  Zero-initialise, then fill in:
 *   conv = 0: out[M][ldc] = (A[M][lda] | A2[M][lda2]) W[N][K]^T, the sources split at column C1 of K (A2 = NULL: one source, C1 ignored);
 *             geglu = 1: W holds 2 N_out rows interleaved in 16-row value / gate groups (gyre_op_repack_linear_weight), N = N_out.
 *   conv = 1: 3x3 convolution of the NHWC image A[B][Hi][Wi][lda] (| A2 [..][lda2], split at channel C1 of Cin), W [N][3][3][Cin]:
 *             stride 1 / 2; pad = 1 (all sides) or 0 (one zero row / column below and right: the (0,1,0,1) pad of a downsampler);
 *             ups = 1: nearest 2x upsample first, of logical size Hup x Wup (0 = 2 Hi x 2 Wi; 2 Hi - 1 / 2 Wi - 1 crops the last row /
 *             column); wrap bit 0 / 1: circular instead of zero padding along x / y.  M, K are derived (B Ho Wo, 9 Cin).
 *   epilogue: + bias[N] (GEGLU: [2 N_out] interleaved) + rowbias[row / rows_per_sample][ld_rowbias] + residual[M][ldr], one rounding.
 *   out_mode = 0: 16-bit rows [M][ldc]; 1: NCHW of out_dtype (GYRE_F32 / BF16 / F16; convolutions); 2: transposed,
 *             out[(b N + col) ldt + tok] with tokens rows per b (linear).  ws / ws_bytes: split-K slab space (may be NULL).
 * lda / lda2 / ldc / ldr = 0 mean the logical widths.  The tile config is the planner's, or the one forced through
 * gyre_debug_force_gemm_cfg.  A plan in K slices needs its slab space in ws (gyre_debug_gemm_plan says how much): too little is
 * GYRE_ERR_WORKSPACE, never a silent run of another configuration.  Bad sizes, strides below the logical width, a missing pointer: GYRE_ERR_INVALID and no launch; a
 * form the chosen kernel does not have: GYRE_ERR_UNSUPPORTED and no launch. */
typedef struct gyre_gemm_test_args {
    int32_t conv, M, K, N, geglu;
    int32_t B, Hi, Wi, Cin, stride, pad, ups, Hup, Wup, wrap;
    int32_t C1, lda, lda2, ldc, ldr;
    int32_t rows_per_sample, ld_rowbias, samples;
    int32_t out_mode, out_dtype, tokens, ldt;
    int32_t colstat_unit;      /* gyre_debug_gemm_plan only: the channel unit its column-statistics answer is for (0: none) */
    const void* A; const void* A2; const void* W;
    const float* bias; const float* rowbias; const void* residual;
    void* out; void* ws; size_t ws_bytes;
    /* the 1x1 shortcut folded into a stride-1 / pad-1 convolution as extra K steps: sc_K more channels of a second image pair
     * sc_A[B][Hi][Wi][sc_lda] (| sc_A2 [..][sc_lda2], split at sc_C1; NULL: one source) behind the conv's; W then holds
     * [N][9 Cin + sc_K] rows (the conv's followed by the shortcut's) and bias the sum of the two.  sc_K = 0: none. */
    const void* sc_A; const void* sc_A2; int32_t sc_K, sc_C1, sc_lda, sc_lda2;
} gyre_gemm_test_args;
int gyre_op_gemm_test(void* stream, const gyre_gemm_test_args* a);
/* Shape query, no device: what gyre_op_gemm_test would launch for `a` under the calling thread's planner state (forced config, tuning
 * switches, scratch buffers).  Pointers are looked at for NULL and for their 16-byte alignment only.  Returns the status the
 * argument check gives; out[12] = tile config, K slices, split-K slab bytes (low / high 32 bits), blocked weights, column-statistics
 * rows (for colstat_unit), row-statistics parts, folded LayerNorm, per-sample weights, folded shortcut, and for the 8-wave
 * tile configs the LDS ring depth (else 0), for convolutions on the 4- and 8-wave configs whether the K loop takes the uniform-tap
 * form (else 0; the other kernels have no tap forms).  out[9] needs the sc_* fields of the folded shortcut. */
int gyre_debug_gemm_plan(const gyre_gemm_test_args* a, int32_t* out);
/* Shape query, no device: would the model runtime run the upsampler (nearest 2x of the NHWC image [B][Hi][Wi][Cin], then a 3x3 / pad 1
 * convolution into N channels) as four 2x2 parity convolutions on composed weights (k_gemm4s)?  Hup / Wup: size of the
 * upsampled image (0 = 2 Hi x 2 Wi; the 2 Hi - 1 crop keeps nine taps), tiling: the request's circular-padding bits, colstat_unit: the
 * channel unit of the GroupNorm statistics asked of the launch (0: none).  Answers for the calling thread's planner state (tuning bits
 * 29 / 30 of gyre_debug_gemm_ablation, batch-invariant mode, forced config).  out[4] = taken (0 / 1), tile config, K slices,
 * column-statistics rows (0: the consumer runs its own statistics pass). */
int gyre_debug_ups4_plan(int B, int Hi, int Wi, int Cin, int N, int Hup, int Wup, int tiling, int colstat_unit, int32_t* out);
/* Tests / tuning only: that upsampler in the four-parity form, one call.  x NHWC [B][Hi][Wi][Cin] storage, w [N][3][3][Cin] storage
 * (gyre_op_repack_conv_weight), bias [N] fp32 or NULL, out [B][2 Hi][2 Wi][N] storage.  scratch: 16 N Cin storage elements, receives
 * the composed weights (four [N][4 Cin] matrices, blocked order) on every call.  splits <= 1: the planner's form for the calling
 * thread's switches; splits >= 2: that many K slices forced (ws: splits x B 2Hi 2Wi N floats; no column statistics).
 * colstat_out: [B 4 Hi Wi / rows][N / colstat_unit][2] floats (rows: gyre_debug_ups4_plan) or NULL.  GYRE_ERR_UNSUPPORTED where the
 * form is not taken (gyre_debug_ups4_plan) - never a nine-tap launch instead. */
typedef struct gyre_upsample_conv_test_args {
    int32_t B, Hi, Wi, Cin, N, splits, colstat_unit;
    const void* x; const void* w; const float* bias;
    void* out; float* colstat_out;
    void* scratch; size_t scratch_bytes;
    void* ws; size_t ws_bytes;
} gyre_upsample_conv_test_args;
int gyre_op_upsample_conv_test(void* stream, const gyre_upsample_conv_test_args* a);
/* The tile-config table: out[4 i ..] = id, rows, columns, kernel family (0 register-staged 4-wave, 1 LDS-DMA 8-wave, 2 pipelined,
 * 3 A-resident, 4 small-problem) of the i-th configuration; at most cap ints are written.  Returns the number of configurations. */
int gyre_debug_gemm_tiles(int32_t* out, int cap);

/* ---- batch-invariant mode ------------------------------------------------
 * The reference asserts that an image does not depend on what shares its batch (tests/batch_independance.py:15-27)
 * and splits a request into sub-batches by available memory (services/generate.py:977-990,1049-1091).  All kernels
 * here are batch-position independent and every GEMM tile configuration sums in the same order, but the split-K
 * factor of the deep (16x16 / 8x8) UNet levels is chosen from the tile count and therefore from the batch size.
 * canonical_samples > 0 plans that factor as if every call held canonical_samples batch entries (16 = the
 * 8-images-with-CFG call of the headline configuration): results become bit-identical for ANY split of a batch
 * over GPUs or sub-batches, while calls much smaller than the canonical size fill the chip less well.
 * 0 (default) = plan for the actual batch.  The setting belongs to the CALLING THREAD (one thread drives one device slot in
 * the reference, manager.py:2107-2139): it affects the forwards and workspace queries that thread issues, nothing else.
 * Returns the previous value. */
int gyre_set_batch_invariant(int canonical_samples);
int gyre_get_batch_invariant(void);

/* ---- single operators (kernel-level parity tests and profiling) --------- */
/* All tensors NHWC / row-major in the library's 16-bit storage type unless noted ("bf16" in the names and comments below reads "fp16"
 * for libgyre_hip_f16.so: gyre_storage_dtype); f32 for norm affine, bias. */
int gyre_op_groupnorm(void* stream, const void* x, const void* x2, int C1, int B, int HW, int C, int groups,
                      const float* gamma, const float* beta, float eps, int silu,
                      void* workspace, size_t workspace_bytes, void* y);
size_t gyre_op_groupnorm_workspace(int B, int HW, int C, int groups);
/* GroupNorm statistics from the PRODUCER of a tensor.  On the UNet's large feature maps the kernels that write a tensor a
 * GroupNorm will read (3x3 convs incl. their split-K reduction, the transformer's proj_out) also leave, per block of `rows`
 * consecutive output rows and per `unit` of consecutive channels, the sum and the sum of squares of the bf16 values they
 * stored: stats_out [M / rows][N / unit][2] f32, fixed summation order, no atomics.  rows is dictated by the kernel the
 * planner picks (returned through rows_out; GYRE_ERR_UNSUPPORTED when that kernel cannot: then the consumer runs its own
 * statistics pass); unit divides every GroupNorm group that will read the tensor - alone or as part of a skip concat.
 * gyre_op_groupnorm_colstats is the consumer: no statistics pass, mean / rstd are finished from the partials of x (and x2) in
 * the prologue of the one launch that normalises.  workspace of the producers: gyre_op_gemm_splitk_bytes (0 = none; for a conv
 * it assumes the square stride-1 geometry sqrt(M / B) x sqrt(M / B) - any other conv: pass at least 4 * 16 * M * N bytes, the largest
 * split factor's slabs).  Non-positive sizes, a unit / rows_per_sample of 0 or one that does not divide N / M: GYRE_ERR_INVALID. */
size_t gyre_op_gemm_splitk_bytes(int conv, int M, int N, int K, int B);
int gyre_op_conv3x3_colstats(void* stream, const void* x, int B, int Hi, int Wi, int Cin, const void* w_repacked, int Cout,
                             const float* bias, const void* residual, int stride, int ups, int unit, void* y, float* stats_out,
                             size_t stats_bytes, void* workspace, size_t workspace_bytes, int* rows_out);
int gyre_op_linear_colstats(void* stream, const void* x, int M, int K, const void* w_bf16_rowmajor, int N, const float* bias,
                            const void* residual, int rows_per_sample, int unit, void* y, float* stats_out, size_t stats_bytes,
                            void* workspace, size_t workspace_bytes, int* rows_out);
int gyre_op_groupnorm_colstats(void* stream, const void* x, const void* x2, int C1, int B, int HW, int C, int groups,
                               const float* gamma, const float* beta, float eps, int silu, const float* cs_x, int cs_x_chunks,
                               const float* cs_x2, int cs_x2_chunks, int unit, void* workspace, size_t workspace_bytes, void* y);
/* The affine-only GroupNorm folded into the Linear that consumes it, up to but not including the GEMM: per sample
 * Wf_out [B][N][C] = W diag(rstd gamma) (16-bit, rounded once) and bf_out [B][N] f32 = bias + W (beta - mean rstd gamma).
 * cs_x != NULL: statistics from the producer's partials ([B][cs_x_chunks][C / unit][2], unit divides C / groups), else the
 * kernel's own statistics pass.  bias may be NULL.  workspace: gyre_op_groupnorm_workspace(B, HW, C, groups) bytes. */
int gyre_op_gn_fold(void* stream, const void* x, int B, int HW, int C, int groups, const float* gamma, const float* beta, float eps,
                    const void* W, const float* bias, int N, const float* cs_x, int cs_x_chunks, int unit,
                    void* workspace, size_t workspace_bytes, void* Wf_out, float* bf_out);
int gyre_op_layernorm(void* stream, const void* x, int M, int C, const float* gamma, const float* beta,
                      float eps, void* y);
/* y[M,N] = x[M,K] @ w[N,K]^T (+bias) (+residual); geglu!=0: w holds [2N,K], y = val*gelu(gate) */
int gyre_op_linear(void* stream, const void* x, int M, int K, const void* w_bf16_rowmajor, int N,
                   const float* bias, const void* residual, int geglu, void* y);
/* y = LayerNorm(x; gamma, beta, eps) @ w^T (+bias) with the normalisation folded into the GEMM: one streaming pass writes each
 * row's (rstd, rstd * mean), the GEMM multiplies the RAW rows by gamma-scaled weights and its epilogue applies
 * rstd * acc - rstd * mean * colsum[n] + bias'[n]; the normalised tensor is never written or re-read.  Folded weights,
 * column constants and row statistics live in `workspace` (gyre_op_ln_linear_workspace(rows of w, K, M) bytes).  This is how
 * the UNet's transformer blocks run norm1 -> Q|K|V, norm2 -> to_q and norm3 -> GEGLU (third-party BasicTransformerBlock,
 * reached from gyre/pipeline/unet/core.py:274).  qkv_tokens > 0: w = [3K][K] rows Q | K | V, y = Q | K ([M][2K]), vt_out = V^T
 * as in gyre_op_qkv.  GYRE_ERR_UNSUPPORTED when the planner's tile configuration for the shape has no folded form (the model
 * then runs the separate gyre_op_layernorm pass). */
size_t gyre_op_ln_linear_workspace(int w_rows, int K, int M);
/* row_parts / n_parts: instead of the streaming statistics pass, take the partial row sums the PRODUCER of x left
 * (gyre_op_linear_rowstats); NULL / 0: run the pass. */
int gyre_op_ln_linear(void* stream, const void* x, int M, int K, const float* gamma, const float* beta, float eps,
                      const void* w_bf16_rowmajor, int N, const float* bias, int geglu, int qkv_tokens, void* vt_out, int ldt,
                      const float* row_parts, int n_parts, void* workspace, size_t workspace_bytes, void* y);
/* gyre_op_linear that also leaves, per row, the (sum, sum of squares) of the bf16-rounded outputs of each of its N tiles:
 * stats_out [parts][M][2] f32, parts = gyre_op_linear_rowstats_parts(...) (0 = the planner's kernel for the shape has no such
 * epilogue -> GYRE_ERR_UNSUPPORTED).  In the UNet the producers of a transformer block's internal tensors (proj_in, the two
 * attention to_out projections, FF2 of a previous block) hand these to the LayerNorm folded into the next GEMM. */
int gyre_op_linear_rowstats_parts(int M, int K, int N, int has_residual);
int gyre_op_linear_rowstats(void* stream, const void* x, int M, int K, const void* w_bf16_rowmajor, int N, const float* bias,
                            const void* residual, void* y, float* stats_out);
/* V^T form used by attention: y[(b*N + n)*ldt + tok] = (x @ w^T + bias)[b*tokens + tok][n] */
int gyre_op_linear_t(void* stream, const void* x, int M, int K, const void* w_bf16_rowmajor, int N,
                     const float* bias, int tokens_per_batch, int ldt, void* y);
/* 3x3 conv NHWC, weights already repacked [Cout][3][3][Cin] bf16; ups!=0 fuses nearest-2x upsample
 * of the input; stride 1|2; pad 1 (pad 0 + bottom/right zero pad when asym!=0, VAE downsample). */
int gyre_op_conv3x3(void* stream, const void* x, int B, int Hi, int Wi, int Cin, const void* w_krsc, int Cout,
                    const float* bias, const void* residual, int stride, int ups, int asym, void* y);
/* A resnet's conv2 with its 1x1 shortcut folded in (round 6): y = conv3x3(x; stride 1, pad 1) + (sx | sx2) w_sc^T + bias + bias_sc in ONE
 * launch - the shortcut's channels are extra K steps of the pipelined 256x320 convolution tile, same accumulators, one rounding.
 * sx [B][H][W][C1], sx2 [B][H][W][C2] or NULL with C2 = 0 (the skip concatenation of an up block is never materialised), w_sc
 * [Cout][C1 + C2] repacked.  Cin, C1, C2 multiples of 64.  ws: Cout * (9 Cin + C1 + C2) * 2 + Cout * 4 + 512 bytes.
 * GYRE_ERR_UNSUPPORTED where the planner's kernel for the shape does not know the form (the model then runs the two launches). */
int gyre_op_conv3x3_shortcut(void* stream, const void* x, int B, int H, int W, int Cin, const void* w_krsc, int Cout, const float* bias,
                             const void* sx, int C1, const void* sx2, int C2, const void* w_sc, const float* bias_sc, void* ws,
                             size_t ws_bytes, void* y);
/* The composed weights of a Transformer2D's proj_out folded into the FF2 of its last block (round 7), as the model handles make them
 * once per weight version: wc_out [C][5C] = [Wp W2 | Wp] in the storage type (fp32 sums over k ascending, one rounding), bc_out [C] =
 * Wp b2 + bp in fp32 (b2 / bp may be NULL).  wp [C][C] and w2 [C][4C] are storage rows (gyre_op_repack_linear_weight); C % 64 == 0. */
int gyre_op_compose_proj_out(void* stream, const void* wp, const void* w2, const float* b2, const float* bp, int C, void* wc_out,
                             float* bc_out);
/* The output convolution of the UNet / VAE decoder (3x3, stride 1, zero padding 1, Cout <= 16) written as NCHW y
 * [B][Cout][H][W] of dtype y_dtype (0 f32, 1 bf16, 2 f16), as the models' last launch does: the dedicated kernel
 * (kernels_conv_out.hip) where Cin % 64 == 0, the tile kernels otherwise; force_tiles != 0 takes the tile kernels anyway. */
int gyre_op_conv3x3_nchw(void* stream, const void* x, int B, int H, int W, int Cin, const void* w_krsc, int Cout,
                         const float* bias, void* y, int y_dtype, int force_tiles);
/* Repack helpers used by the tests to build the layouts above from PyTorch-layout f32 tensors */
int gyre_op_repack_conv_weight(void* stream, const float* w_oihw, int Cout, int Cin, int KH, int KW, int Cin_pad,
                               void* w_krsc_bf16);
/* The same repack as gyre_unet_set_weight runs it for a weight that carries a folded factor (the softmax scale in to_k): source of
 * any gyre_dtype, every value round(scale * w), the product and the rounding exactly as the store does them.  The tests compare
 * gyre_op_repack_lora's bits with it. */
int gyre_op_repack_conv_weight_scaled(void* stream, const void* w_oihw, int dtype, int Cout, int Cin, int KH, int KW, int Cin_pad,
                                      float scale, void* w_krsc);
int gyre_op_repack_linear_weight(void* stream, const float* w_oi, int O, int I, int geglu_interleave, void* w_bf16);
int gyre_op_repack_bias(void* stream, const float* b, int n, int geglu_interleave, float* out);
/* The repack of gyre_unet_set_weight_lora as an operator (gyre_op_repack_delta restricted to GYRE_DELTA_LORA terms): base (O x I x KH x KW, base_dtype) and n_pairs LoRA factor pairs ->
 * out [O][KH][KW][I_pad] in the storage type (pad columns zero; KH = KW = 1 for a matrix; geglu != 0: the 16-row value / gate
 * interleave of gyre_op_repack_linear_weight, the up factor indexed by the SOURCE row), every value
 * round(scale_p * (base + sum_j scale_j up_j down_j)) with the sum in fp32: r ascending inside a pair, pairs in argument order.
 * I_pad >= I and a multiple of 4; out is caller-owned, O * KH * KW * I_pad elements. */
int gyre_op_repack_lora(void* stream, const void* base, int base_dtype, int O, int I, int KH, int KW, int I_pad,
                        int geglu_interleave, float scale_p, int n_pairs, const gyre_lora_pair* pairs, void* out);
/* The repack of gyre_unet_set_weight_delta as an operator (arguments as gyre_op_repack_lora, terms as gyre_delta_term), and the
 * core contraction that prepares a Tucker form:  out[a][c][t] = sum_b core[a][b][t] * right[b][c],  core [A][B][T] and right [B][C]
 * of their own gyre_dtype, out fp32 [A][C][T], b ascending with fused multiply-adds.  core(mid, down) is the down operand of a LoCon
 * with a mid tensor, core(t, wb) that of a LoHa / LoKr Tucker form, and T = 1 gives w1 = w1a @ w1b. */
int gyre_op_repack_delta(void* stream, const void* base, int base_dtype, int O, int I, int KH, int KW, int I_pad,
                         int geglu_interleave, float scale_p, int n_terms, const gyre_delta_term* terms, void* out);
int gyre_op_lyco_core(void* stream, const void* core, int core_dtype, const void* right, int right_dtype, int A, int B, int C, int T,
                      float* out);
/* The same sum on a plain matrix, for a weight that lives outside the native store (a CLIP text encoder's nn.Linear):
 *   out[o][i] = round_out( base[o][i] + sum_j scale_j * D_j[o][i] ),  summed in fp32 in term order, one rounding to out_dtype
 * base [O][I] row-major of base_dtype, out [O][I] row-major of out_dtype - GYRE_F32 (stored as computed), GYRE_BF16 or GYRE_F16
 * (round to nearest even), whichever storage type the library was built for.  Terms and their checks as gyre_op_repack_delta with
 * KH = KW = 1; no interleave, no pad columns, no folded factor.  n_terms == 0 with out_dtype == base_dtype copies base bit for bit
 * (how an adapter is taken off).  I % 4 == 0, out aligned to 4 elements, and out must not overlap base or an operand (the caller
 * keeps the original): GYRE_ERR_INVALID otherwise.  Every check precedes the launch and a refused call writes nothing. */
int gyre_op_merge_delta(void* stream, const void* base, int base_dtype, int O, int I, int n_terms, const gyre_delta_term* terms,
                        void* out, int out_dtype);
/* o[B,Nq,H*D] = softmax(q k^T * D^-1/2) v ; q[B,Nq,H*D] (ldq), k[B,Nk,H*D] (ldk), vt[B,H*D,ldvt] (V transposed) */
int gyre_op_attention(void* stream, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt,
                      int B, int heads, int Nq, int Nk, int D, void* o, int ldo);
/* Fused Q|K|V projection as the UNet self-attention runs it: x[M,C] (bf16) times w_qkv[3C,C] (rows Q | K | V, repacked
 * with gyre_op_repack_linear_weight) -> qk_out[M,2C] row-major and vt_out[M/tokens][C][ldt] = V transposed per batch
 * entry.  Needs an 8-wave tile configuration whose wave tiles align with column 2C (GYRE_ERR_UNSUPPORTED otherwise;
 * the model then issues two GEMMs). */
int gyre_op_qkv(void* stream, const void* x, int M, int C, const void* w_qkv, int tokens, void* qk_out, void* vt_out, int ldt);
/* Same, k_prescaled != 0: k already holds k * log2(e)/sqrt(D) (the UNet folds that factor into its to_k weights in
 * fp32 before their bf16 rounding), which lets the kernel take exp2 of the matrix-core output directly. */
int gyre_op_attention_ex(void* stream, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt,
                         int B, int heads, int Nq, int Nk, int D, void* o, int ldo, int k_prescaled);
/* ToMe merge of one self-attention's keys / values: k[B,N,ldk], v[B,N,ldv] (bf16 rows of C channels) ->
 * k_out[B,N-r,C], vt_out[B,C,ldvt] (values transposed, columns >= N-r zero); optional order_out / node_idx_out [B,N/2]
 * (int32, dev) receive the a-token ranking and every a token's best match.  r is clipped to N / 2. */
/* Input gradient of gyre_vae_decode (clipguided.py:366-386 decodes latent cut-outs under autograd): writes the decoded
 * image and d_z = (d image / d z)^T d_image. */
size_t gyre_vae_decode_vjp_workspace_bytes(gyre_vae* h, int B, int h_lat, int w_lat);
int gyre_vae_decode_vjp(gyre_vae* h, void* stream, const void* z_nchw, int z_dtype, int B, int h_lat, int w_lat,
                        const void* d_image_nchw, int d_dtype, void* workspace, size_t workspace_bytes,
                        void* image_out_nchw, int out_dtype, void* dz_out_nchw, int dz_dtype);

/* ---- input-gradient kernels, exposed for the parity tests (tests/test_gpu_vjp.py); activations / gradients bf16 ----
 * groupnorm_bwd: x (|| x2) is the forward INPUT, dy[B,HW,C] the gradient of the (activated) output; dx[B,HW,C1],
 *   dx2[B,HW,C-C1]; addend (optional, [B,HW,C1]) is added to dx.
 * layernorm_bwd: same for rows of [M,C].  geglu_bwd: pre[M,2F] in the packed column order of
 *   gyre_op_repack_linear_weight(geglu=1), dy[M,F], dpre[M,2F].
 * attention_bwd: q/k/v/o/d_o row-major [B,N,ld] with head h at column h*D (v is NOT transposed here); dk == NULL
 *   computes dq only (cross-attention). */
size_t gyre_op_groupnorm_bwd_workspace(int B, int HW, int C, int groups);
int gyre_op_groupnorm_bwd(void* stream, const void* x, const void* x2, int C1, int B, int HW, int C, int groups,
                          const float* gamma, const float* beta, float eps, int silu, const void* dy, const void* addend,
                          void* workspace, size_t workspace_bytes, void* dx, void* dx2);
int gyre_op_layernorm_bwd(void* stream, const void* x, const void* dy, int M, int C, const float* gamma, float eps,
                          const void* addend, void* dx);
int gyre_op_geglu_bwd(void* stream, const void* pre, const void* dy, int M, int F, void* dpre);
size_t gyre_op_attention_bwd_workspace(int B, int heads, int Nq, int Nk, int D);
int gyre_op_attention_bwd(void* stream, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv,
                          const void* o, int ldo, const void* d_o, int lddo, int B, int heads, int Nq, int Nk, int D,
                          int k_prescaled, void* workspace, size_t workspace_bytes, void* dq, int lddq, void* dk, int lddk,
                          void* dv, int lddv);
size_t gyre_op_tome_workspace(int B, int N, int C);
int gyre_op_tome_merge(void* stream, const void* k, int ldk, const void* v, int ldv, int B, int N, int C, int r,
                       void* workspace, size_t workspace_bytes, void* k_out, void* vt_out, int ldvt,
                       int32_t* order_out, int32_t* node_idx_out);
/* gyre_op_tome_merge plus two optional outputs: dstlist_out [B,N/2] (int32, dev; entry k < r = the b token the k-th ranked a
 * token was merged into) and vrows_out [B,N-r,C] (the merged values row-major, what the backward pass reads). */
int gyre_op_tome_merge_ex(void* stream, const void* k, int ldk, const void* v, int ldv, int B, int N, int C, int r,
                          void* workspace, size_t workspace_bytes, void* k_out, void* vt_out, int ldvt,
                          int32_t* order_out, int32_t* node_idx_out, int32_t* dstlist_out, void* vrows_out);
/* Adjoint of the merge for one merged tensor: dy[B,N-r,C] -> dx[B,N,ldx]; every original token receives the gradient of the row
 * it went into, divided by that row's token count.  order / dstlist as gyre_op_tome_merge_ex returned them, r = the EFFECTIVE r
 * (1 <= r <= N / 2, not clipped here), inv_scratch [B,N/2] int32. */
int gyre_op_tome_unmerge(void* stream, const void* dy, int B, int N, int C, int r, const int32_t* order, const int32_t* dstlist,
                         int32_t* inv_scratch, void* dx, int ldx);
/* The time-embedding chain, fp32 rows.  timestep_embedding: out[B,dim] = the diffusers sinusoidal embedding of t[B] (int64, dev),
 * [cos | sin] when flip, exponent -ln(10000) i / (dim / 2 - shift); dim even.  rowvec_linear: out[B,N] (row stride ldo) =
 * f(x[B,K]) w[N,K]^T + bias, w in 16-bit storage row-major, f = SiLU when act_in_silu (for B > 4 it is applied to x IN PLACE,
 * for B <= 4 x is left as it is); K % 8 == 0.  timestep_linear: rowvec_linear of the embedding (K = dim, dim % 8 == 0), one
 * launch for B <= 4; emb_scratch [B,dim] f32 is needed above that. */
int gyre_op_timestep_embedding(void* stream, const int64_t* t, int B, int dim, int flip, float shift, float* out);
int gyre_op_rowvec_linear(void* stream, float* x, int B, int K, const void* w, const float* bias, int N, int act_in_silu,
                          float* out, int ldo);
int gyre_op_timestep_linear(void* stream, const int64_t* t, int B, int dim, int flip, float shift, float* emb_scratch,
                            const void* w, const float* bias, int N, float* out, int ldo);
/* The cross-attention block of a transformer block as ONE launch (round 6, kernels_xattn.hip; the model runs it for the attn2 module of
 * diffusers' BasicTransformerBlock at SD1.x's 64x64 level): out = softmax(LayerNorm(x) Wq^T . K^T) V Wo^T + bo + x and, if row_stats
 * is not NULL, per row the (sum, sum of squares) of the rounded outputs.  x [M][C] = the rows BEFORE the LayerNorm (M = B * tokens),
 * wq / wo [C][C] repacked, k [B][Nk][C] already multiplied by log2(e) / sqrt(C / heads), vt [B][C][ldvt] = V transposed (ldvt >= Nk
 * rounded up to 8).  ws: gyre_op_ln_linear_workspace(C, C, M) bytes.  GYRE_ERR_UNSUPPORTED outside the kernel's domain (C = 320,
 * 8 heads, Nk <= 80, tokens % 128 == 0, M / 128 >= 256). */
int gyre_op_cross_attention_block(void* stream, const void* x, int M, int tokens, int C, int heads, const float* gamma,
                                  const float* beta, float eps, const void* wq, const void* k_prescaled, const void* vt, int Nk,
                                  int ldvt, const void* wo, const float* bo, void* ws, size_t ws_bytes, void* out, float* row_stats);
int gyre_op_nchw_to_nhwc(void* stream, const void* x, int dtype, int B, int C, int HW, int Cpad, void* y_bf16);
/* The element-wise kernels of the T2I adapter (kernels_t2i.hip).  pixel_unshuffle8: x NCHW [B][c][H][W] of a runtime dtype -> y NHWC
 * storage [B][H/8][W/8][64 c] in torch.nn.PixelUnshuffle(8) channel order.  avgpool2: NHWC storage [B][H][W][C] -> [B][H/2][W/2][C]
 * (C % 8 == 0; fp32 sum, one rounding).  relu: in place on n storage elements (n % 8 == 0). */
int gyre_op_pixel_unshuffle8(void* stream, const void* x, int dtype, int B, int c, int H, int W, void* y);
int gyre_op_avgpool2(void* stream, const void* x, int B, int H, int W, int C, void* y);
int gyre_op_relu(void* stream, void* x, size_t n);
/* The element-wise kernels of the ControlNet (kernels_ctrl.hip).  silu: x * sigmoid(x) in place on n storage elements (n % 8 == 0),
 * fp32 math, one rounding; NaN stays NaN, a finite input stays finite.  ctrl_emit: the residual hand-off described at
 * gyre_ctrl_forward over f NHWC storage [B][HW][Cpad] (the first C channels; Cpad % 8 == 0). */
int gyre_op_silu(void* stream, void* x, size_t n);
int gyre_op_ctrl_emit(void* stream, const void* f, int B, int C, int HW, int Cpad, float scale, int accumulate, void* out,
                      int out_dtype, int out_B, int out_b0);
/* The masked forms behind gyre_ctrl_bind_slot / gyre_ctrl_forward_slot, mask fp32 [mask_B][HW] with mask_B == 1 or B.
 * ctrl_emit_masked: out = rnd(fl(fl(scale f) mask[b or 0][p]) [+ old]).  nchw_to_nhwc_masked: y NHWC storage [B][HW][Cpad] =
 * rnd(x[b][c][p] mask[b or 0][p]) from x NCHW of a runtime dtype, pad channels zero. */
int gyre_op_ctrl_emit_masked(void* stream, const void* f, int B, int C, int HW, int Cpad, float scale, int accumulate, void* out,
                             int out_dtype, int out_B, int out_b0, const float* mask, int mask_B);
int gyre_op_nchw_to_nhwc_masked(void* stream, const void* x, int dtype, int B, int C, int HW, int Cpad, const float* mask, int mask_B,
                                void* y);
/* The kernels of the RRDBNet upscaler (kernels_rdb.hip).  rdb_tile: the output tile (pixels) of the dense-block convolution.
 * rdb_conv: one launch of it; GYRE_ERR_UNSUPPORTED outside its domain (NT other than 32 / 64, Cin % 32, strides or c0 not multiples of
 * 8, unaligned buffers, grid limits) and GYRE_ERR_INVALID for bad arguments, nothing written either way.  rdb_epilogue: the same
 * epilogue in place over x[pix][c0 .. c0 + N_live) of npix pixels with stride ldo (acc = the stored value).  pixel_unshuffle: x NCHW
 * [B][c][H][W] of a runtime dtype -> y NHWC storage [B][H / r][W / r][c r^2 rounded up to 32] in torch pixel_unshuffle channel
 * order (r = 1, 2, 4; the padding channels are zeros). */
int gyre_op_rdb_tile(int* th, int* tw);
int gyre_op_rdb_conv(void* stream, const gyre_rdb_conv_args* args);
int gyre_op_rdb_epilogue(void* stream, void* x, int c0, int ldo, int N_live, size_t npix, const gyre_rdb_epilogue* epi);
int gyre_op_pixel_unshuffle(void* stream, const void* x, int dtype, int B, int c, int H, int W, int r, void* y);
/* The kernels of the SwinIR upscaler (kernels_swin.hip).  win_bias: relative_position_bias_table [225][heads] fp32 -> bias_out, heads *
 * 4096 floats in the attention kernel's order.  win_attn: shifted-window attention over 8 x 8 windows, head dim 30 stored as 32: qkv
 * [B H W][ld_qkv] storage, token order, q / k / v of head h at columns 32 h / 32 (heads + h) / 32 (2 heads + h); o [B H W][ld_o], head h
 * written at [30 h, 30 h + 30), every other element keeps its bits; bias = win_bias's output; shift 0 or 4 (0 when H == 8 or W == 8);
 * the scale 30^-1/2 multiplies the fp32 dot products.  GYRE_ERR_UNSUPPORTED / GYRE_ERR_INVALID outside the domain, nothing written.
 * ln_live: LayerNorm over the first C channels of M rows with stride ldx; y rows of stride ldy: values in [0, C), zeros in [C, ldy).
 * swin_act: in place on n storage elements (n % 8 == 0), mode 0 = erf GELU, mode 1 = leaky ReLU with the given slope.
 * swin_entry: x NCHW [B][3][HW] -> y NHWC storage [B][HW][8] = (x - mean[c]) * range, channels 3 .. 7 zero.  swin_exit: x NHWC storage
 * [B][HW][ldx] -> y NCHW [B][3][HW] = x / range + mean[c]. */
int gyre_op_win_bias(void* stream, const float* table, int heads, float* bias_out);
int gyre_op_win_attn(void* stream, const void* qkv, int ld_qkv, void* o, int ld_o, const float* bias, int B, int H, int W, int heads,
                     int shift);
int gyre_op_ln_live(void* stream, const void* x, int ldx, size_t M, int C, const float* gamma, const float* beta, float eps, void* y,
                    int ldy);
int gyre_op_swin_act(void* stream, void* x, size_t n, int mode, float slope);
int gyre_op_swin_entry(void* stream, const void* x, int dtype, int B, size_t HW, const float* mean3, float range, void* y);
int gyre_op_swin_exit(void* stream, const void* x, int ldx, int B, size_t HW, const float* mean3, float range, void* y, int dtype);
/* The kernels of the HAT upscaler (kernels_hat.hip).  hat_attn: attention over 16 x 16 windows, head dim 30 stored as 32, qkv / o laid
 * out as for win_attn; table = the relative-position table itself, fp32 [961][heads] (mode 0, self-attention: 256 keys of the window
 * under shift 0 or 8, mask from the window position) or [1521][heads] (mode 1, overlapping cross-attention: the 24 x 24 keys around the
 * window, zero k / v outside the image, the reference's index modulo 1521; shift must be 0).  H and W multiples of 16, 1 to 8 heads.
 * chan_pool: pool[b][c] = mean over HW of x[b][.][c] (c < C <= 256) in a fixed order; partial = gyre_op_chan_pool_workspace bytes.
 * chan_gate: s[b][c] = scale * sigmoid(w2[c] . relu(w1 pool[b] + b1) + b2[c]), zeros in [C, ld_s); w1 [Cs][C], w2 [C][Cs], Cs <= 8.
 * scale_add: y[b][p][c] += c2[b][p][c] * s[b][c] for c < Cn (a multiple of 8).  pixel_shuffle2: out[b][2 y + i][2 x + j][c] =
 * x[b][y][x][4 c + 2 i + j] for c < Co (a multiple of 8), NHWC, exact.  GYRE_ERR_UNSUPPORTED / GYRE_ERR_INVALID outside the domain. */
int gyre_op_hat_attn(void* stream, const void* qkv, int ld_qkv, void* o, int ld_o, const float* table, int mode, int B, int H, int W,
                     int heads, int shift);
size_t gyre_op_chan_pool_workspace(int B, size_t HW, int C);
int gyre_op_chan_pool(void* stream, const void* x, int ld, int B, size_t HW, int C, float* partial, float* pool);
int gyre_op_chan_gate(void* stream, const float* pool, int B, int C, int Cs, const float* w1, const float* b1, const float* w2,
                      const float* b2, float scale, float* s, int ld_s);
int gyre_op_scale_add(void* stream, void* y, int ldy, const void* c2, int ldc, const float* s, int ld_s, int B, size_t HW, int Cn);
int gyre_op_pixel_shuffle2(void* stream, const void* x, int ld_x, int B, int H, int W, int Co, void* out, int ld_out);
/* The kernels of the line-art hinter (kernels_inorm.hip), one launch each.
 * inorm_stats: stats[b][c] = (mean, rstd) over the HW rows (stride ld) of x, biased variance, c < C = 64 / 128 / 256, fp32 in a fixed
 * order; partial = gyre_op_inorm_workspace bytes.  inorm_apply: see gyre_inorm_apply_args.  tconv_compose: a ConvTranspose2d(3, stride 2,
 * padding 1, output_padding 1) weight [Cin][Cout][3][3] of a runtime dtype -> its sub-pixel matrix [4 Cout][4 Cin] in the storage type,
 * rows (a, b, co), columns (dy, dx, ci), 7 of the 16 blocks zero.  conv7_in: reflection padding 3 + 7x7 conv of the 8-channel NHWC entry
 * tensor (3 live) into NHWC 64; w [64][3][7][7] of w_dtype, w_scratch 64 * 49 * 8 storage elements.  conv7_out: 7x7 conv of the pad-3
 * NHWC image [B][Ho + 6][Wo + 6][64] into one NCHW plane of out_dtype, + bias, optional sigmoid; w [1][64][7][7], w_scratch 49 * 64. */
/* conv3x3_valid: the planner convolution in the form the line-art graph runs over a reflect-padded image - no padding, stride 1,
 * y NHWC [B][Hi - 2][Wi - 2][Cout] from x NHWC [B][Hi][Wi][Cin], w [Cout][3][3][Cin] storage, planned as if each sample ran alone. */
int gyre_op_conv3x3_valid(void* stream, const void* x, int B, int Hi, int Wi, int Cin, const void* w, int Cout, const float* bias, void* y);
size_t gyre_op_inorm_workspace(int B, size_t HW, int C);
int gyre_op_inorm_stats(void* stream, const void* x, int ld, int B, size_t HW, int C, float eps, float* partial, float* stats);
int gyre_op_inorm_apply(void* stream, const gyre_inorm_apply_args* args);
int gyre_op_tconv_compose(void* stream, const void* w, int dtype, int Cin, int Cout, void* out);
int gyre_op_conv7_in(void* stream, const void* x8, int B, int H, int W, const void* w, int w_dtype, void* w_scratch, const float* bias,
                     void* out);
int gyre_op_conv7_out(void* stream, const void* xp, int B, int Ho, int Wo, const void* w, int w_dtype, void* w_scratch, const float* bias,
                      int sigmoid, void* out, int out_dtype);
/* The kernels of the HED edge detector (kernels_hed.hip), one launch each.
 * hed_entry: x NCHW [B][3][H][W] of dtype -> y NHWC storage [B][H + 68][W + 68][8], the image inside a 34-pixel zero border, channels
 * 3 .. 7 zero.  hed_tail: x NHWC storage [B][Hs][Ws][C] (C = 64 / 128 / 256 / 512; a stage's last convolution before its ReLU) ->
 * pool [B][ceil(Hs / 2)][ceil(Ws / 2)][C] = relu(max over the 2x2 ceil-mode window) (null: not written) and so [B][Hs][Ws] fp32 =
 * bias[0] + sum_c w[c] relu(x[c]).  hed_fuse: see gyre_hed_fuse_args. */
int gyre_op_hed_entry(void* stream, const void* x, int dtype, int B, int H, int W, void* y);
int gyre_op_hed_tail(void* stream, const void* x, int B, int Hs, int Ws, int C, const float* w, const float* bias, void* pool, float* so);
int gyre_op_hed_fuse(void* stream, const gyre_hed_fuse_args* args);
/* The kernels of the MLSD line detector (kernels_mlsd.hip), one launch each; activations NHWC storage, channel counts and pixel
 * strides in multiples of 8, fp32 arithmetic in a fixed order, one rounding.
 * mlsd_fold: see gyre_mlsd_fold_args.  mlsd_entry: x NCHW [B][4][H][W] of dtype -> y [B][H / 2][W / 2][32] = relu6(conv3x3 stride 2 +
 * bias), zero padding on the right / bottom only (output o reads inputs 2 o .. 2 o + 2); w [9][4][32] storage.
 * dwconv3: y = relu6(depthwise 3x3 (x) + bias), w [9][C] storage; stride 1 with zero padding 1 -> [B][H][W][C], stride 2 with the
 * right / bottom padding -> [B][H / 2][W / 2][C]; relu6_in: relu6 is applied to x as it is read.
 * upsample2_ac: y[..][0 .. C) (pixel stride ldy) = bilinear x2, align_corners=True, of x [B][H][W] (pixel stride ldx); relu_in: relu on
 * the reads.  dconv3_d5: y = relu(conv3x3 with dilation 5 and zero padding 5 (x) + bias), [B][H][W][64] -> the same, w [64][9][64].
 * mlsd_act: in place, relu (relu6 != 0: relu6) over the first C channels of rows of pitch ld.  mlsd_relu_add: y = relu(y) + x over n
 * elements.  mlsd_exit: out NCHW [B][9][H][W] of out_dtype = channels 7 .. 15 of x [B][H][W][16]. */
int gyre_op_mlsd_fold(void* stream, const gyre_mlsd_fold_args* args);
int gyre_op_mlsd_entry(void* stream, const void* x, int dtype, int B, int H, int W, const void* w, const float* bias, void* y);
int gyre_op_dwconv3(void* stream, const void* x, int B, int H, int W, int C, const void* w, const float* bias, int stride, int relu6_in,
                    void* y);
int gyre_op_upsample2_ac(void* stream, const void* x, int B, int H, int W, int C, int ldx, int relu_in, void* y, int ldy);
int gyre_op_dconv3_d5(void* stream, const void* x, int B, int H, int W, const void* w, const float* bias, void* y);
int gyre_op_mlsd_act(void* stream, void* x, size_t rows, int C, int ld, int relu6);
int gyre_op_mlsd_relu_add(void* stream, void* y, const void* x, size_t n);
int gyre_op_mlsd_exit(void* stream, const void* x, int B, int H, int W, void* out, int out_dtype);
/* The kernels of the token-sequence T2I networks (StyleAdapter, CoAdapterFuser; kernels_seq.hip), one launch each.
 * seq_attn: multi-head self-attention over the packed in_proj output.  qkv [N L][ld_qkv] storage, sample-major rows (row n L + l), q / k
 * / v of head h at columns h D / heads D + h D / 2 heads D + h D; o [N L][ld_o], head h written at [h D, h D + D), every other element
 * keeps its bits.  softmax(D^-1/2 q k^T) v over the L keys of the sample: fp32 logits and statistics, probabilities and outputs rounded
 * once; no mask, no bias.  D = 32, 64, 96 or 128 and L <= gyre_op_seq_attn_max_len(D) (1120 / 576 / 384 / 288; 0 for another D):
 * GYRE_ERR_UNSUPPORTED beyond, GYRE_ERR_INVALID for bad arguments, nothing written either way.
 * quick_gelu: x sigmoid(1.702 x) in place on n storage elements (n % 8 == 0), fp32 math, one rounding.
 * fuser_pool: x NCHW storage [N][C][HW] -> out[n][c] = silu(mean over HW), storage rows of stride ld_out >= C, a fixed summation order.
 * fuser_gain: out[n][c][.] = x[n][c][.] (alpha[n][c] + 1) (accumulate 0) or out += the same (accumulate 1) over NCHW storage maps;
 * alpha fp32 rows of stride ld_a >= C; each fp32 operation rounds on its own, then one rounding to storage. */
int gyre_op_seq_attn_max_len(int D);
int gyre_op_seq_attn(void* stream, const void* qkv, int ld_qkv, void* o, int ld_o, int N, int L, int heads, int D);
int gyre_op_quick_gelu(void* stream, void* x, size_t n);
int gyre_op_fuser_pool(void* stream, const void* x, int N, int C, size_t HW, void* out, int ld_out);
int gyre_op_fuser_gain(void* stream, const void* x, const float* alpha, int ld_a, int N, int C, size_t HW, void* out, int accumulate);
/* Device-side memcpy-rate probe used by bench.py to calibrate the HBM roofline on the box. */
int gyre_op_copy_probe(void* stream, const void* src, void* dst, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GYRE_HIP_H */
