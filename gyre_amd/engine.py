"""Engine-level drop-in: the reference's ``UnifiedPipeline`` call contract over the native pipeline.

An existing Gyre server selects it in engines.yaml:

    - id: "stable-diffusion-v1-5-mi355x"
      class: "gyre_amd.engine.GyreUnifiedPipeline"
      model: "@sd15"
      overrides:
        unet: {class: "gyre_amd.modules.GyreHipUNet"}
        vae:  {class: "gyre_amd.modules.GyreHipVAE"}

and everything above it stays the reference's own code: ``EngineManager`` builds the object from the loaded modules
(manager.py:1712-1783: ``Class(**modules)``), wraps it in ``DiffusionPipelineWrapper`` (pipeline_wrapper.py:164-397), the
gRPC servicer (services/generate.py:992-1152) calls the wrapper with the request's kwargs and turns the returned tensors
into PNG artifacts.  What this class has to honour is therefore exactly what the wrapper touches:

  * constructor keywords = module names (vae, text_encoder, tokenizer, unet, scheduler, inpaint_unet, ...);
    ``pipeline_modules()`` so that ``PipelineWrapper.activate(device)`` can swap in per-device clones (:96-131)
  * ``scheduler`` attribute: the wrapper injects the sampler chosen by the request (:255-267) - a k-diffusion sampler
    callable or a diffusers scheduler object; it is mapped back to the native sampler of the same name
  * ``progress_bar`` attribute: wrapped around the step iterable, raises ``ProgressBarAbort`` on cancellation (:26-47)
  * ``__call__`` keywords of ``UnifiedPipeline.__call__`` (unified_pipeline.py:1722-1790) - the wrapper filters its
    kwargs by this signature (:269-286) - returning ``(images [B,3,H,W] in 0..1, nsfw flags)`` for
    ``output_type="tensor", return_dict=False`` (:2512-2534)
  * ``set_options`` with the reference's option names (unified_pipeline.py:1538-1629)
  * no-op memory knobs (attention / VAE slicing, xformers): 288 GB of HBM3E, the whole batch stays resident.

Hint images handled by a T2I adapter (gyre_amd/t2i.py GyreHipT2IAdapter through the engine's ``hintset_manager``) run natively:
the adapter once per request, its states added inside the UNet on every step (gyre_amd/hints.py); style adapters and co-adapters with
their fuser likewise (GyreHipT2IStyleAdapter / GyreHipT2IFuser: style tokens extend the text context once per request).  Hint images handled by a ControlNet
(gyre_amd/controlnet.py GyreHipControlNet) run natively as well: the hint image and the text context are bound once per request, the
control model runs once per UNet evaluation and its residuals go to the UNet's residual inputs (schedulers.UNetWithControlnet).
ControlNet hints also run under hires fix (on by default: every leaf of the tree has its own copy of the hint on its own bind slot of
the control model), with an alpha plane as their mask, and in an inpaint request (``mask_image``): with a grafted inpaint pair
and next to a 9-channel inpaint UNet, where the control model sees latents x mask channel (unified_pipeline.py:1016-1024).  As in the
reference (for_model(mask=None), :2026) the request's ``mask_image`` is not the hint's mask.
Features outside the native hot path raise NotImplementedError (-> gRPC UNIMPLEMENTED, services/exception_to_grpc.py): depth maps /
depth UNets, foreign hint handlers, masked T2I hints, T2I hints together with hires fix / grafted inpaint, any hint together
with CLIP guidance / shard_devices.  CLIP guidance
is implemented (gyre_amd/clipguided.py over the native input-gradient sweeps).  ``lora=`` takes LoRA files (kohya-ss, diffusers) and,
as the reference routes them (unified_pipeline.py:2210-2233: what ``detect_lora_type`` refuses goes to ``apply_lycoris``), LyCORIS files
(LoCon, LoHa, LoKr, full diff; gyre_amd/lycoris.py): one attach for the whole request, every touched weight repacked once on the
device, taken off again at the start of the next request.  IA3, DyLoRA, sparse-bias LyCORIS modules and cloneofsimo LoRA files raise
NotImplementedError.  The text side of a request (gyre_amd/text_adapters.py, SD1.x / 2.x engines): the ``lora_te_`` entries of the same
files are merged into the text encoder's Linear weights (one gyre_op_merge_delta per touched weight, scaled by the ``"text_encoder"`` /
``"*"`` weights as the reference's loop leaves them; a file with nothing but ``lora_te_`` entries works), and ``token_embeddings=``
(textual inversion) adds its tokens to the request's own copy of the tokenizer and its rows to the token table; both are taken off at
the start of the next request, before the prompts are encoded.  SDXL engines (``text_time``) raise NotImplementedError for
``token_embeddings`` and ignore ``lora_te*`` entries.  The safety checker stays the host module the
manager loaded; it is RUN exactly as the reference runs it (``_safety_check``), never skipped silently.
"""
from __future__ import annotations

import copy
import functools
from typing import Any, Callable, List, Optional

import torch

from . import clipguided as CG
from . import lora as LR
from . import lycoris as LY
from . import text_adapters as TA
from .pipeline import GyrePipeline
from .text import LPWTextEmbedder

# sampler callables (k-diffusion function names, reference samplers.py:47-67) / diffusers scheduler classes (:24-45)
_K_NAMES = {"sample_lms": "lms", "sample_euler": "euler", "sample_euler_ancestral": "euler_a", "sample_dpm_2": "dpm_2",
            "sample_dpm_2_ancestral": "dpm_2_a", "sample_heun": "heun", "sample_dpm_fast": "dpm_fast",
            "sample_dpm_adaptive": "dpm_adaptive", "sample_dpmpp_2s_ancestral": "dpmpp_2s_a", "sample_dpmpp_sde": "dpmpp_sde",
            "sample_dpmpp_2m": "dpmpp_2m"}
_D_NAMES = {"DDIMScheduler": "ddim", "PNDMScheduler": "plms", "LMSDiscreteScheduler": "lms", "EulerDiscreteScheduler": "euler",
            "EulerAncestralDiscreteScheduler": "euler_a", "DPM2DiscreteScheduler": "dpm_2",
            "DPM2AncestralDiscreteScheduler": "dpm_2_a", "HeunDiscreteScheduler": "heun"}


def sampler_name(scheduler: Any) -> str:
    """The native sampler for what the reference's wrapper injected as ``pipeline.scheduler``."""
    if isinstance(scheduler, str):
        return scheduler
    fn = scheduler
    while isinstance(fn, functools.partial):
        fn = fn.func
    name = getattr(fn, "__name__", None)
    if name in _K_NAMES:
        return _K_NAMES[name]
    cls = type(scheduler).__name__
    if cls == "DPMSolverMultistepScheduler":
        cfg = getattr(scheduler, "config", None)
        order = cfg.get("solver_order", 2) if isinstance(cfg, dict) else getattr(cfg, "solver_order", 2)
        return f"dpmsolverpp_{int(order) if isinstance(order, int) else 2}"
    if cls in _D_NAMES:
        return _D_NAMES[cls]
    raise NotImplementedError(f"Scheduler not implemented: {scheduler!r}")


class GyreUnifiedPipeline:
    # reference UnifiedPipeline._meta (unified_pipeline.py:1265): both sampler families; weights stay resident (no offload)
    _meta = {"diffusers_capable": True, "kdiffusion_capable": True, "offload_capable": False}

    def __init__(self, vae, text_encoder, tokenizer, unet, scheduler=None, safety_checker=None, feature_extractor=None,
                 clip_model=None, clip_tokenizer=None, inpaint_unet=None, inpaint_text_encoder=None, depth_unet=None,
                 depth_text_encoder=None, hintset_manager=None, text_encoder_2=None, tokenizer_2=None,
                 force_zeros_for_empty_prompt: bool = True, **_unused):
        self.vae, self.text_encoder, self.tokenizer, self.unet = vae, text_encoder, tokenizer, unet
        # SDXL (BASELINE configs[3]; an extension - the reference has no SDXL): the second text tower of the published
        # pipeline layout (model_index.json: text_encoder_2 / tokenizer_2).  Requests are routed by the UNet's
        # addition_embed_type == "text_time" (gyre_amd/text.py SDXLTextConditioner, sdxl_time_ids)
        self.text_encoder_2, self.tokenizer_2 = text_encoder_2, tokenizer_2
        self.force_zeros_for_empty_prompt = force_zeros_for_empty_prompt
        self.scheduler, self.inpaint_unet = scheduler, inpaint_unet
        self.safety_checker, self.feature_extractor = safety_checker, feature_extractor
        self.clip_model, self.clip_tokenizer = clip_model, clip_tokenizer
        self.hintset_manager, self.depth_unet = hintset_manager, depth_unet
        self.inpaint_text_encoder = inpaint_text_encoder
        self.progress_bar: Optional[Callable] = None
        self._grafted_inpaint: Any = False
        self._hires_fix, self._hires_threshold_fraction = True, 0.0333
        self._hires_oos_fraction, self._hires_image_oos_fraction = 0.6, 1.0
        self._text_embedding_layer = "final"
        self._tome = 0
        self._shard_devices: list = []       # engine option "shard_devices": fan one request over these device slots
        self._shard_bit_exact = False
        self._executor = None
        self._lora_uploads: list = []        # lora.Factors of the last four LoRA / LyCORIS tensors mappings seen (_lora_factors)
        self._text_uploads: list = []        # ... and their text-encoder sides (text_adapters.TextFactors, _text_factors)
        self.clip_default_config = CG.ClipGuidanceConfig()

    # ---- what PipelineWrapper / DiffusionPipelineWrapper touch -----------------------------------------------------------
    def pipeline_modules(self):
        for name in ("vae", "text_encoder", "text_encoder_2", "unet", "inpaint_unet"):
            m = getattr(self, name, None)
            if isinstance(m, torch.nn.Module):
                yield name, m

    @property
    def execution_device(self) -> torch.device:
        return next(self.unet.parameters()).device

    device = execution_device

    def to(self, device):
        for name, m in list(self.pipeline_modules()):
            setattr(self, name, m.to(device))
        return self

    def enable_attention_slicing(self, *_a, **_k): pass
    def disable_attention_slicing(self, *_a, **_k): pass
    def enable_vae_slicing(self): pass
    def disable_vae_slicing(self): pass
    def enable_xformers_memory_efficient_attention(self, *_a, **_k): pass
    def disable_xformers_memory_efficient_attention(self): pass

    def set_options(self, options: dict) -> None:
        """Engine ``options:`` of engines.yaml (reference unified_pipeline.py:1538-1629)."""
        for key, value in options.items():
            if key == "hires":
                if isinstance(value, bool):
                    self._hires_fix = value
                else:
                    for sk, sv in value.items():
                        if sk == "enable":
                            self._hires_fix = bool(sv)
                        elif sk == "oos_fraction":
                            self._hires_oos_fraction = float(sv)
                        elif sk == "image_oos_fraction":
                            self._hires_image_oos_fraction = float(sv)
                        elif sk == "threshold_fraction":
                            self._hires_threshold_fraction = float(sv)
                        else:
                            raise ValueError(f"Unknown option {sk}: {sv} passed as part of hires settings")
            elif key == "grafted_inpaint":
                self._grafted_inpaint = value if isinstance(value, dict) else bool(value)
            elif key == "tome":
                self._tome = int(value) if value else 0
            elif key == "clip_skip":
                self._text_embedding_layer = "penultimate" if value else "final"
            elif key in ("xformers", "vae_tiling", "structured_diffusion"):
                pass                                       # memory knobs / deprecated: accepted, nothing to do
            elif key == "clip":                            # unified_pipeline.py:1591-1623
                cfg = self.clip_default_config
                for sk, sv in (value or {}).items():
                    if sk in ("unet_grad", "vae_grad"):
                        pass                               # native weights never receive gradients; only the sample does
                    elif sk in ("vae_cutouts", "approx_cutouts", "gradient_length"):
                        setattr(cfg, sk, int(sv))
                    elif sk == "no_cutouts":
                        cfg.no_cutouts = bool(sv)
                    elif sk in ("guidance_scale", "gradient_threshold", "gradient_maxloss"):
                        setattr(cfg, sk, float(sv))
                    elif sk == "guidance_base":
                        if str(sv) not in ("guided", "mixed"):
                            raise ValueError("Guidance base must be one of 'mixed' or 'guided'")
                        cfg.guidance_base = str(sv)
                    else:
                        raise ValueError(f"Unknown option {sk}: {sv} passed as part of clip settings")
            elif key == "shard_devices":
                # Extension (north_star: "request batches shard data-parallel across the 8 GPUs of one node"): the images of
                # ONE request are split over these devices with the reference's batched_seeds rule and run concurrently from
                # one host thread + HIP stream per device inside this process (gyre_amd/executor.py); weights are replicated
                # on first use.  {"devices": [...], "bit_exact": true} additionally plans split-K batch-invariantly so that
                # the result equals the single-device run bit for bit.
                devs = value.get("devices", []) if isinstance(value, dict) else (value or [])
                self._shard_bit_exact = bool(value.get("bit_exact", False)) if isinstance(value, dict) else False
                self._shard_devices = [torch.device(d if not isinstance(d, int) else f"cuda:{d}") for d in devs]
                self._executor = None
            elif key == "grafted_depth":
                if value:
                    raise NotImplementedError(f"option {key!r} is outside the native hot path")
            else:
                raise ValueError(f"Unknown option {key}: {value} passed to UnifiedPipeline")

    # ---- text -------------------------------------------------------------------------------------------------------------
    def _embed(self, prompt, negative_prompt, B, num_images_per_prompt, do_cfg, max_embeddings_multiples, tokenizer=None):
        """tokenizer: the request's own copy when it carries token embeddings (default: self.tokenizer)."""
        def frags(p):                                       # str | Prompt | list | PromptBatch -> list of [(text, weight)] / str
            if p is None:
                return None
            if hasattr(p, "as_tokens") and hasattr(p, "prompts"):
                return p.as_tokens()
            if hasattr(p, "as_tokens"):
                return [p.as_tokens()]
            if isinstance(p, (list, tuple)):
                return [q.as_tokens() if hasattr(q, "as_tokens") else q for q in p]
            return [p]
        pos = frags(prompt)
        neg = frags(negative_prompt) or [""] * len(pos)
        if len(neg) == 1 and len(pos) > 1:
            neg = neg * len(pos)
        te, dev = self.text_encoder, self.execution_device
        layer = self._text_embedding_layer

        def encode(ids):
            final = layer == "final"
            out = te(input_ids=ids.to(dev), output_hidden_states=not final, return_dict=True)
            if final:
                return out.last_hidden_state.float()
            tower = getattr(te, "text_model", te)
            return tower.final_layer_norm(out.hidden_states[-2]).float()
        encode.device = dev
        tok = self.tokenizer if tokenizer is None else tokenizer

        def tokenize(text):
            text = TA.replace_text(tok, text)               # a multi-vector embedding's <name> -> its sub-tokens, before tokenising
            return tok(text, add_special_tokens=False)["input_ids"] if callable(tok) else tok.encode(text)[1:-1]
        emb = LPWTextEmbedder(encode, tokenize, max_embeddings_multiples)
        cond, unc = emb.get_embeddings(pos, neg if do_cfg else None)
        rep = lambda t: None if t is None else t.repeat_interleave(num_images_per_prompt, dim=0)
        return rep(cond), rep(unc)

    def _embed_sdxl(self, prompt, negative_prompt, B, num_images_per_prompt, do_cfg, max_embeddings_multiples, height, width):
        """SDXL conditioning: context of both text towers [B,77k,2048], pooled text_embeds [B,1280] and time_ids [B,6]
        (gyre_amd/text.py SDXLTextConditioner; published SDXL-base scheme, not in the reference)."""
        from .text import SDXLTextConditioner, sdxl_time_ids
        if self.text_encoder_2 is None or self.tokenizer_2 is None:
            raise ValueError("an SDXL UNet (addition_embed_type 'text_time') needs text_encoder_2 and tokenizer_2")

        def frags(p):
            if p is None:
                return None
            if hasattr(p, "as_tokens") and hasattr(p, "prompts"):
                return p.as_tokens()
            if hasattr(p, "as_tokens"):
                return [p.as_tokens()]
            return list(p) if isinstance(p, (list, tuple)) else [p]
        pos = frags(prompt)
        neg = frags(negative_prompt)        # None stays None: "no negative prompt" conditions on zeros, an explicit "" is encoded

        def mk(tok):
            return lambda text: tok(text, add_special_tokens=False)["input_ids"] if callable(tok) else tok.encode(text)[1:-1]
        dev = self.execution_device
        pad2 = getattr(self.tokenizer_2, "pad_token_id", 0)
        cnd = SDXLTextConditioner(self.text_encoder, mk(self.tokenizer), self.text_encoder_2, mk(self.tokenizer_2), dev,
                                  max_embeddings_multiples, self.force_zeros_for_empty_prompt,
                                  pad_1=getattr(self.tokenizer, "pad_token_id", None), pad_2=0 if pad2 is None else pad2)
        cond, pooled, unc, upooled = cnd(pos, neg, do_cfg)
        rep = lambda t: None if t is None else t.repeat_interleave(num_images_per_prompt, dim=0)
        cond, pooled, unc, upooled = rep(cond), rep(pooled), rep(unc), rep(upooled)
        ids = sdxl_time_ids(cond.shape[0], height, width, device=dev)
        added = {"text_embeds": pooled, "time_ids": ids}
        uadded = {"text_embeds": upooled, "time_ids": ids} if do_cfg else None
        return cond, unc, added, uadded

    # ---- CLIP guidance request (unified_pipeline.py:1876-1909, 1927-1940, 2373-2395) ----------------------------------------
    def _clip_request(self, prompt, clip_prompt, B, num_images_per_prompt, scale, base, glen, gthr, gmax, vae_cutouts,
                      approx_cutouts, no_cutouts) -> dict:
        if scale is not None and self.clip_model is None:
            print("Warning: CLIP guidance passed to a pipeline without a CLIP model. It will be ignored.")
            scale = None
        if not scale:
            return {}
        cfg = copy.copy(self.clip_default_config)
        cfg.guidance_scale = scale
        if base is not None:
            cfg.guidance_base = base
        if glen is not None:
            cfg.gradient_length = glen
        if gthr is not None:
            cfg.gradient_threshold = gthr
        if gmax is not None:
            cfg.gradient_maxloss = gmax
        if vae_cutouts is not None:
            cfg.vae_cutouts = vae_cutouts
        if approx_cutouts is not None:
            cfg.guidance_scale = approx_cutouts      # sic: the reference assigns approx_cutouts to guidance_scale (:1899-1900)
        if no_cutouts is not None:
            cfg.no_cutouts = no_cutouts

        def texts(p):
            if hasattr(p, "as_unweighted_string"):
                t = p.as_unweighted_string()
                return t if isinstance(t, list) else [t]
            items = p if isinstance(p, (list, tuple)) else [p]
            return [q.as_unweighted_string() if hasattr(q, "as_unweighted_string") else
                    (q if isinstance(q, str) else " ".join(f[0] for f in q)) for q in items]
        strings = texts(clip_prompt if clip_prompt is not None else prompt)
        if len(strings) * num_images_per_prompt != B:
            raise ValueError(f"clip_prompt has batch size {len(strings)}, but prompt has batch size {B // num_images_per_prompt}. "
                             "They need to match.")
        tok = self.clip_tokenizer if self.clip_tokenizer is not None else self.tokenizer
        te_cfg = getattr(self.text_encoder, "config", None)
        max_pos = getattr(te_cfg, "max_position_embeddings", 77)
        if hasattr(tok, "model_max_length"):
            ids = tok(strings, padding="max_length", max_length=min(tok.model_max_length, max_pos), truncation=True,
                      return_tensors="pt").input_ids
        else:                                       # bare callable tokenizer (tests): BOS + tokens + EOS, padded with EOS
            bos, eos = getattr(te_cfg, "bos_token_id", 49406), getattr(te_cfg, "eos_token_id", 49407)
            rows = []
            for s_ in strings:
                body = list(tok(s_, add_special_tokens=False)["input_ids"])[:max_pos - 2]
                rows.append([bos] + body + [eos] * (max_pos - 1 - len(body)))
            ids = torch.tensor(rows, dtype=torch.long)
        feats = CG._features(self.clip_model.get_text_features(ids.to(self.execution_device)))
        return dict(clip_guidance_scale=scale, clip_config=cfg,
                    clip_text_embeddings=feats.repeat_interleave(num_images_per_prompt, dim=0))

    def _lora_factors(self, tensors):
        """The uploaded factors of one LoRA or LyCORIS tensors mapping (lora.upload_factors, or lycoris.upload_factors for what
        detect_lora_type refuses - the reference's routing, unified_pipeline.py:2212-2216), remembered per mapping OBJECT: the reference's
        manager keeps a loaded LoRA's dict alive and hands the same object to every request that names it, so its factors go to
        the device once.  Identity-keyed, per UNet object whose shapes the upload was checked against (the entry keeps the mapping
        referenced, its address cannot be recycled), the four most
        recently used sets are kept."""
        dev = self.unet.device
        cache = self._lora_uploads                          # [(tensors mapping, unet the shapes were checked against, lora.Factors)]
        for i, (src, net, f) in enumerate(cache):
            if src is tensors and net is self.unet and f.device == dev:
                cache.append(cache.pop(i))
                return f
        lyco = LY.is_lycoris(tensors)
        if not lyco and LR.detect_lora_type(tensors) == "cloneofsimo":
            raise NotImplementedError("cloneofsimo LoRA files need lora_diffusion's module search order (not vendored)")
        if dev.type != "cuda":
            self.unet._sync(dev)                            # raises: the native UNet has no CPU path
        f = (LY if lyco else LR).upload_factors(self.unet, tensors, dev)
        cache.append((tensors, self.unet, f))
        del cache[:-4]
        return f

    def _text_factors(self, text_encoder, tensors):
        """The text-encoder side of one LoRA / LyCORIS tensors mapping (text_adapters.upload_text_factors), remembered like
        _lora_factors: per mapping OBJECT and encoder object, the four most recently used."""
        dev = TA._device_of(text_encoder)
        cache = self._text_uploads
        for i, (src, te, f) in enumerate(cache):
            if src is tensors and te is text_encoder and f.device == dev:
                cache.append(cache.pop(i))
                return f
        f = TA.upload_text_factors(text_encoder, tensors, dev)
        cache.append((tensors, text_encoder, f))
        del cache[:-4]
        return f

    def _text_encoders(self) -> list:
        """Every distinct text encoder a request may use (the reference's all_text_encoders, unified_pipeline.py:2187-2188)."""
        out = []
        for te in (self.text_encoder, getattr(self, "inpaint_text_encoder", None)):
            if te is not None and not any(te is o for o in out):
                out.append(te)
        return out

    def _text_side(self, lora_specs, token_embeddings):
        """The text side of a request (unified_pipeline.py:1855-1868, 2190-2233), in front of the prompt encoding: what the previous
        request left on every text encoder goes (attached lora_te_ terms, added token rows), then this request's token embeddings
        and the lora_te_ entries of its ``lora_specs = [(tensors, weights)]`` go on.  Returns the tokenizer to encode the prompts
        with: self.tokenizer, or the request's own copy with the embeddings' tokens added."""
        encoders = self._text_encoders()
        tokenizer = self.tokenizer
        if token_embeddings:
            for te in encoders:
                TA.check_ti(te, token_embeddings)           # a wrong dimension raises before anything changed
        for te in encoders:
            TA.detach(te)
            TA.match_encoder_to_tokenizer(self.tokenizer, te)
        if token_embeddings:
            tokenizer = copy.deepcopy(self.tokenizer)       # tokens added for this call only; clip_tokenizer stays as it is
            flattened = TA.apply_ti_to_tokenizer(tokenizer, token_embeddings)
            for te in encoders:
                TA.apply_ti_to_encoder(tokenizer, te, flattened)
        text_specs = [(t, w) for t, w in lora_specs if TA.has_text_keys(t)]
        if text_specs:
            for te in encoders:
                TA.attach(te, [(self._text_factors(te, t), TA.text_scale(w)) for t, w in text_specs])
        return tokenizer

    def _hints(self, hint_images, mask_image, inpaint_request: bool = False) -> list:
        """The reference's hint loop (unified_pipeline.py:1994-2047) for what is native: every hint image needs exactly one model
        from the hintset manager and that model must be a GyreHipT2IAdapter (-> hints.T2IHint, or hints.CoAdapterHint with the
        hintset's fuser when it was loaded as a co-adapter), a GyreHipT2IStyleAdapter (-> hints.StyleHint with the hintset's clip_model,
        feature_extractor, fuser and the hint's clip_layer) or a GyreHipControlNet (-> hints.ControlNetHint; same priority and weight mapping).  Depth hints routed to a depth UNet and foreign handlers stay
        NotImplementedError; a hint type nobody handles is the reference's EnvironmentError.  inpaint_request: the caller hands
        ``mask_image`` on to a pipeline that serves ControlNet hints next to it (``__call__`` does); as in the reference
        (for_model(mask=None), unified_pipeline.py:2026) the request's mask is never the hint's own mask.  Without it a ControlNet
        hint together with a mask keeps raising, as it did before the pipeline could."""
        from .controlnet import GyreHipControlNet
        from .hints import CoAdapterHint, ControlNetHint, StyleHint, T2IHint
        from .t2i import GyreHipT2IAdapter, GyreHipT2IStyleAdapter
        hints = []
        for hint_image in hint_images or ():
            hint_type = hint_image.hint_type
            weight = 1.0 if hint_image.weight is None else hint_image.weight
            priority = hint_image.priority
            if hint_type == "depth" and getattr(self, "depth_unet", None) is not None:
                raise NotImplementedError("depth hints routed to a depth UNet are outside the native hot path")
            handler_models = self.hintset_manager.for_type(hint_type, None) if self.hintset_manager else None
            if not handler_models:
                raise EnvironmentError(f"Pipeline doesn't know how to handle hint image of type {hint_type}")
            models = dict(handler_models)
            extras = {extra: models.pop(extra, None) for extra in ("clip_model", "feature_extractor", "fuser")}
            if len(models) != 1:
                raise ValueError(f"Unknown set of hint models: {models.keys()}")
            _, model = models.popitem()
            if isinstance(model, GyreHipControlNet):
                if mask_image is not None and not inpaint_request:
                    raise NotImplementedError("ControlNet hints together with a mask need a caller that serves them (inpaint_request=True)")
                hints.append(ControlNetHint(model, hint_image.image, mask=None, weight=weight, soft_injection=priority != "balanced",
                                            cfg_only=priority == "hint"))
                continue
            common = dict(mask=None, weight=weight, soft_injection=priority != "balanced", cfg_only=priority == "hint")
            if isinstance(model, GyreHipT2IStyleAdapter):          # t2i-adapter-style, coadapter-style (UnifiedPipelineHint_T2i, style path)
                hints.append(StyleHint(model, hint_image.image, extras["clip_model"], extras["feature_extractor"], fuser=extras["fuser"],
                                       clip_layer=getattr(hint_image, "clip_layer", None), **common))
                continue
            if not isinstance(model, GyreHipT2IAdapter):
                raise NotImplementedError(f"hint model {type(model).__name__} (ControlNet and foreign adapters are outside the native hot path)")
            if getattr(model, "_coadapter_type", False):           # coadapter/*: the states go through the hintset's fuser
                if mask_image is not None:
                    raise NotImplementedError("co-adapter hints together with a mask")
                hints.append(CoAdapterHint(model, hint_image.image, extras["fuser"], **common))
                continue
            hints.append(T2IHint(model, hint_image.image, **common))
        return hints

    # ---- the generation call (keywords of reference UnifiedPipeline.__call__, unified_pipeline.py:1722-1790) ---------------
    @torch.no_grad()
    def __call__(self, prompt, height: int = 512, width: int = 512, image=None, mask_image=None, outmask_image=None,
                 depth_map=None, hint_images=None, strength: Optional[float] = None, num_inference_steps: int = 50,
                 guidance_scale: float = 7.5, negative_prompt=None, num_images_per_prompt: int = 1,
                 prediction_type: Optional[str] = "epsilon", eta: Optional[float] = None, churn: Optional[float] = None,
                 churn_tmin: Optional[float] = None, churn_tmax: Optional[float] = None, sigma_min: Optional[float] = None,
                 sigma_max: Optional[float] = None, karras_rho: Optional[float] = None, scheduler_noise_type: str = "normal",
                 generator=None, latents=None, max_embeddings_multiples: int = 3, output_type: str = "pil",
                 return_dict: bool = True, callback=None, callback_steps: int = 1, clip_guidance_scale: Optional[float] = None,
                 clip_guidance_base: Optional[str] = None, clip_gradient_length: Optional[int] = None,
                 clip_gradient_threshold: Optional[float] = None, clip_gradient_maxloss: Optional[float] = None,
                 clip_prompt=None, vae_cutouts: Optional[int] = None, approx_cutouts: Optional[int] = None, no_cutouts=False,
                 run_safety_checker: bool = True, lora=None, token_embeddings=None,
                 hires_fix=None, hires_oos_fraction=None, tiling=False, debug_latent_tags=None, debug_latent_prefix="",
                 cfg_execution: str = "parallel"):
        if depth_map is not None:
            raise NotImplementedError("depth-map conditioning (depth UNet) is outside the native hot path")
        from .hints import ControlNetHint
        all_hints = self._hints(hint_images, mask_image, inpaint_request=True)
        t2i_hints = [h for h in all_hints if not isinstance(h, ControlNetHint)]
        controlnet_hints = [h for h in all_hints if isinstance(h, ControlNetHint)]
        if all_hints and len(self._shard_devices) > 1:
            raise NotImplementedError("hint images together with shard_devices (the adapter states and the bound control models live on one device slot)")
        if tiling not in (False, None, True, "x", "y", "xy"):
            raise ValueError(f"tiling must be True, False, 'x', 'y' or 'xy', got {tiling!r}")
        if tiling and clip_guidance_scale:
            raise NotImplementedError("tiling together with CLIP guidance (the native input-gradient sweep has no circular convolutions)")
        if scheduler_noise_type not in (None, "normal", "brownian"):
            raise ValueError(f"scheduler_noise_type must be 'normal' or 'brownian', got {scheduler_noise_type!r}")
        # `latents`: accepted and IGNORED, as in the reference - UnifiedPipeline.__call__ declares and documents the keyword
        # (unified_pipeline.py:1749,1807-1810) but never reads it; start latents always come from the per-image generators.
        # A caller that passes start latents gets an image unrelated to them, so say it once per call (parity kept, silence not)
        if latents is not None:
            import warnings
            warnings.warn("GyreUnifiedPipeline: the `latents` argument is accepted for signature compatibility and ignored (as in the "
                          "reference, unified_pipeline.py:1749); start latents come from the per-image generators / seeds",
                          RuntimeWarning, stacklevel=2)
        if self.scheduler is None:
            raise ValueError("no scheduler injected")
        n_prompts = len(prompt.prompts) if hasattr(prompt, "prompts") else (len(prompt) if isinstance(prompt, (list, tuple)) else 1)
        B = n_prompts * num_images_per_prompt
        if generator is None:
            generators = [torch.Generator("cpu").manual_seed(torch.seed() % (2 ** 31)) for _ in range(B)]
        else:
            generators = list(generator) if isinstance(generator, (list, tuple)) else [generator]
            if len(generators) != B:
                if len(generators) == 1 and B > 1:
                    raise ValueError("one torch.Generator per image is required for batch-independent results")
                raise ValueError(f"Generator passed as a list, but list length does not match batch size {B}")
        do_cfg = guidance_scale > 1.0
        sdxl = getattr(getattr(self.unet, "config", None), "addition_embed_type", None) == "text_time"
        added = uadded = None
        lora_specs = []
        for spec in (lora if isinstance(lora, (list, tuple)) else [lora]) if lora else ():
            tensors, weights = (spec if isinstance(spec, (list, tuple)) else (spec, {}))
            lora_specs.append((tensors, weights))
        if sdxl:
            # SDXL files name two towers (lora_te1_ / lora_te2_), a key space the reference does not have: their text side stays
            # ignored, and token embeddings (one vector per tower) stay refused
            if token_embeddings:
                raise NotImplementedError("textual-inversion token embeddings on an SDXL engine (two text towers)")
        else:
            tokenizer = self._text_side(lora_specs, token_embeddings)
        if sdxl:
            cond, unc, added, uadded = self._embed_sdxl(prompt, negative_prompt, B, num_images_per_prompt, do_cfg,
                                                        max_embeddings_multiples, height, width)
        else:
            cond, unc = self._embed(prompt, negative_prompt, B, num_images_per_prompt, do_cfg, max_embeddings_multiples, tokenizer)
        if strength is None:
            strength = 0.8
        dev = self.execution_device
        pipe = GyrePipeline(self.unet, self.vae, None, device=dev, inpaint_unet=self.inpaint_unet,
                            grafted_inpaint=self._grafted_inpaint, clip_model=self.clip_model,
                            feature_extractor=self.feature_extractor)
        clip_kw = self._clip_request(prompt, clip_prompt, B, num_images_per_prompt, clip_guidance_scale, clip_guidance_base,
                                     clip_gradient_length, clip_gradient_threshold, clip_gradient_maxloss, vae_cutouts,
                                     approx_cutouts, no_cutouts)
        pipe.hires_fix, pipe.hires_threshold_fraction = self._hires_fix, self._hires_threshold_fraction
        pipe.hires_oos_fraction, pipe.hires_image_oos_fraction = self._hires_oos_fraction, self._hires_image_oos_fraction
        # reference set_tiling_mode (unified_pipeline.py:1696-1712, called per request at :1845): every Conv2d of every module
        # pads circularly for this request - the native modules switch their conv gather
        for m in (self.unet, self.inpaint_unet, self.vae):
            if m is not None and hasattr(m, "set_tiling"):
                m.set_tiling(tiling or False)
        for u in (self.unet, self.inpaint_unet):
            if u is None:
                continue
            LR.remove_lora_from_model(u)                    # the reference strips leftovers on every call (:2190-2200)
            LR.detach_loras(u)                              # ... and what the previous request attached on the device path
            if hasattr(u, "set_tome"):                      # the reference patches ToMe into self.unet only (:1580-1584)
                u.set_tome(self._tome if u is self.unet else 0)
        if lora_specs:                                      # (a file with lora_te_ entries only touches no UNet weight: an empty attach)
            specs = []
            for i, (tensors, weights) in enumerate(lora_specs):
                scale = (weights or {}).get("unet", 1.0) if isinstance(weights, dict) else 1.0
                specs.append((tensors, f"request-{i}", scale))
            if hasattr(self.unet, "_sync"):                 # native UNet: merged on the device, each touched weight repacked once
                LR.attach_loras(self.unet, [(self._lora_factors(t), lid, sc) for t, lid, sc in specs])
            else:
                for t, lid, sc in specs:
                    (LY.apply_lycoris if LY.is_lycoris(t) else LR.apply_lora)(self.unet, t, lid, sc)
        steps_seen = []

        def cb(info):
            steps_seen.append(info.get("i", len(steps_seen)))
            if callback is not None and len(steps_seen) % max(callback_steps, 1) == 0:
                callback(len(steps_seen) - 1, info.get("t"), info.get("x"))
        if self.progress_bar is not None:
            # the wrapper's tqdm object polls the stop event on every update (ProgressBarWrapper, pipeline_wrapper.py:26-47)
            bar = self.progress_bar(total=num_inference_steps)
            cb_inner = cb

            def cb(info, _b=bar):
                cb_inner(info)
                if hasattr(_b, "update"):
                    _b.update(1)
        to_dev = lambda t: None if t is None else t.to(dev)
        request = dict(generators=generators, text_embeddings=cond, uncond_embeddings=unc, height=height, width=width,
                       num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                       sampler=sampler_name(self.scheduler), image=to_dev(image), mask_image=to_dev(mask_image),
                       strength=strength, karras_rho=karras_rho, eta=eta, cfg_execution=cfg_execution,
                       hires_fix=hires_fix, hires_oos_fraction=hires_oos_fraction,
                       prediction_type=prediction_type or "epsilon", churn=churn, churn_tmin=churn_tmin or 0.0,
                       churn_tmax=churn_tmax if churn_tmax is not None else float("inf"), sigma_min=sigma_min,
                       sigma_max=sigma_max, scheduler_noise_type=scheduler_noise_type or "normal", **clip_kw)
        if sdxl:
            request.update(added_cond=added, uncond_added_cond=uadded)
        if t2i_hints:
            request.update(t2i_hints=[h.to(dev) for h in t2i_hints])
        if controlnet_hints:
            request.update(controlnet_hints=[h.to(dev) for h in controlnet_hints])
        if len(self._shard_devices) > 1 and B > 1 and not clip_kw and not lora and not self._tome and not tiling:
            # one request over several device slots (engine option "shard_devices"); progress / cancellation are polled once
            # per request here: the replicas run their loops concurrently and a per-step callback has no single owner.
            # (CLIP guidance couples the batch through its flat-loss stop; per-request LoRA / ToMe patch one
            # UNet object - such requests run on this slot alone)
            images = self._sharded(pipe, request, outmask_image=to_dev(outmask_image), image=to_dev(image))
            cb({"i": num_inference_steps - 1})
        else:
            images = pipe(callback=cb, outmask_image=to_dev(outmask_image), **request)
        images = images.float().cpu()                       # reference: result_image.cpu() ... BCHW 0..1 (:2512-2531)
        images, nsfw = self._safety_check(images, run_safety_checker)
        if output_type == "pil":
            images = self.numpy_to_pil(images.permute(0, 2, 3, 1).numpy())
        elif output_type not in ("tensor", "pt"):
            raise ValueError(f"output_type {output_type!r}")
        if not return_dict:
            return images, nsfw
        from types import SimpleNamespace
        return SimpleNamespace(images=images, nsfw_content_detected=nsfw)

    def _sharded(self, pipe, request, outmask_image=None, image=None):
        from . import images as I
        from .executor import DeviceSlotExecutor
        ex = self._executor
        if ex is not None and (ex.source.unet is not self.unet or ex.source.vae is not self.vae
                               or ex.source.inpaint_unet is not self.inpaint_unet or ex.stale(self._shard_devices)):
            ex = None       # other module objects, new weights (load_state_dict / .to / .half / LoRA) or another device list
        if ex is None:
            pipe0 = GyrePipeline(self.unet, self.vae, None, device=self.execution_device, inpaint_unet=self.inpaint_unet,
                                 grafted_inpaint=self._grafted_inpaint)
            self._executor = DeviceSlotExecutor.replicate(pipe0, self._shard_devices)
        ex = self._executor
        for rep in ex.pipelines:                 # per-request engine settings follow the replicas
            rep.grafted_inpaint = self._grafted_inpaint
            rep.hires_fix, rep.hires_threshold_fraction = pipe.hires_fix, pipe.hires_threshold_fraction
            rep.hires_oos_fraction, rep.hires_image_oos_fraction = pipe.hires_oos_fraction, pipe.hires_image_oos_fraction
        latents = ex(bit_exact=self._shard_bit_exact, **request)
        result = ex.decode(latents)
        if image is not None and outmask_image is not None:         # unified_pipeline.py:2493-2510
            src = image if image.ndim == 4 else image[None]
            om = outmask_image if outmask_image.ndim == 4 else outmask_image[None]
            result = I.outmask_composite(result, src.to(result.device), om.to(result.device))
        return result

    @staticmethod
    def numpy_to_pil(images):
        """NHWC 0..1 floats -> PIL images (what the reference inherits from DiffusionPipeline.numpy_to_pil)."""
        from PIL import Image
        if images.ndim == 3:
            images = images[None]
        return [Image.fromarray(im) for im in (images * 255).round().astype("uint8")]

    def _safety_check(self, images: torch.Tensor, run_safety_checker: bool):
        """The host-side NSFW check of the reference (unified_pipeline.py:2512-2523): whenever a checker is loaded it sees
        the finished images - ``feature_extractor`` on the PIL images, then ``safety_checker(images=<NHWC numpy>,
        clip_input=<pixel_values in the text-embedding dtype>)`` - and its (possibly blacked-out) images and per-image flags
        are what the call returns.  The server's default ``nsfw_behaviour`` is "block" (server.py:660) and relies on it."""
        if not run_safety_checker or self.safety_checker is None:
            return images, [False] * images.shape[0]
        if self.feature_extractor is None:
            raise ValueError("a safety_checker needs the pipeline's feature_extractor")
        result_numpy = images.permute(0, 2, 3, 1).numpy()
        dev = self.execution_device
        te_param = next(iter(self.text_encoder.parameters()), None) if hasattr(self.text_encoder, "parameters") else None
        dtype = te_param.dtype if te_param is not None else torch.float32
        clip_input = self.feature_extractor(self.numpy_to_pil(result_numpy), return_tensors="pt").to(dev)
        result_numpy, nsfw = self.safety_checker(images=result_numpy, clip_input=clip_input.pixel_values.to(dtype))
        if isinstance(result_numpy, torch.Tensor):
            result_numpy = result_numpy.float().cpu().numpy()
        import numpy as np
        return torch.from_numpy(np.ascontiguousarray(result_numpy)).permute(0, 3, 1, 2), [bool(f) for f in nsfw]
