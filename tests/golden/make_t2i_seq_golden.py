"""Build-container script: EXECUTES the reference's StyleAdapter and CoAdapterFuser and records what they computed in
t2i_seq_vectors.npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_t2i_seq_golden.py

  * gyre/pipeline/t2i_adapter/adapter.py ``StyleAdapter`` / ``CoAdapterFuser`` at the tiny configurations (gyre_amd.config.tiny_t2i_style /
    tiny_t2i_fuser) on synthetic_state_dict(shapes, seed) weights and seeded inputs: the state-dict key names and the outputs of each case;
  * the same classes at the reference's default configurations: key names and shapes only;
  * unet/core.py ``UNetWithT2I`` (``__init__`` and the context extension of ``__call__``) over fake hints and a fake UNet that records
    its keyword arguments, and unified_pipeline.py ``UnifiedPipelineHint_T2i.style_call`` over a fake ``vision_model``.

The file holds inputs, seeds, configurations, outputs and key lists only; weights are regenerated from the seed
(tests/test_t2i_seq_host.py).  Third-party packages the reference imports but this path never runs are stubbed (make_golden._install).
Nothing here ships."""
import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STYLE_SEED, FUSER_SEED = 31, 32


def main():
    import make_golden as mg
    mg._install()
    from gyre.pipeline.t2i_adapter import adapter as A
    from gyre_amd import config as gcfg, weights
    import t2i_seq_ref as R

    out = {}
    # key names and shapes of the default-size networks
    for name, net, shapes in (("style_default", A.StyleAdapter(num_token=8), weights.t2i_style_param_shapes(gcfg.t2i_style_config())),
                              ("fuser_default", A.CoAdapterFuser(), weights.t2i_fuser_param_shapes(gcfg.t2i_fuser_config()))):
        sd = net.state_dict()
        out[f"{name}.keys"] = np.array(list(sd.keys()))
        out[f"{name}.shapes"] = np.array(json.dumps([list(v.shape) for v in sd.values()]))
        assert {k: tuple(v.shape) for k, v in sd.items()} == dict(shapes), name

    scfg = gcfg.tiny_t2i_style()
    style = A.StyleAdapter(**{k: v for k, v in scfg.items() if k != "type"}).eval()
    out["style.keys"] = np.array(list(style.state_dict().keys()))
    style.load_state_dict(weights.synthetic_state_dict(weights.t2i_style_param_shapes(scfg), STYLE_SEED))
    out["style.cfg"], out["style.seed"] = np.array(json.dumps(dict(scfg))), np.array(STYLE_SEED)
    for N, S in R.STYLE_CASES:
        x = R.style_input(N, S, scfg["width"])
        with torch.no_grad():
            out[f"style.{N}x{S}.out"] = style(x).numpy()

    fcfg = gcfg.tiny_t2i_fuser()
    fuser = A.CoAdapterFuser(**{k: (list(v) if k == "unet_channels" else v) for k, v in fcfg.items() if k != "type"}).eval()
    out["fuser.keys"] = np.array(list(fuser.state_dict().keys()))
    fuser.load_state_dict(weights.synthetic_state_dict(weights.t2i_fuser_param_shapes(fcfg), FUSER_SEED))
    out["fuser.cfg"], out["fuser.seed"] = np.array(json.dumps({**fcfg, "unet_channels": list(fcfg["unet_channels"])})), np.array(FUSER_SEED)
    for name, spec in R.FUSER_CASES.items():
        feats = R.fuser_inputs(spec, fcfg)
        with torch.no_grad():
            maps, seq = fuser({k: v for k, v in feats})
        out[f"fuser.{name}.spec"] = np.array(json.dumps(spec))
        for i, m in enumerate(maps or []):
            out[f"fuser.{name}.map{i}"] = m.numpy()
        if seq is not None:
            out[f"fuser.{name}.seq"] = seq.numpy()
    # UNetWithT2I.__init__ and the context extension of __call__ over fake hints that return seeded states (tests/t2i_seq_ref.hint_states)
    # and a fake UNet that records its keyword arguments; the fuser is the reference's own, with the weights above
    from gyre.pipeline.unet import core as UC

    class FakeHint:
        def __init__(self, cotype, kind, T, seed, cfg_only):
            self.cotype, self.cfg_only, self.fuser = cotype, cfg_only, fuser if cotype else None
            self.state = R.hint_states(kind, T, seed, fcfg)

        def coadapter_type(self):
            return self.cotype

        def __call__(self):
            return self.state

    class FakeUNet:
        def __call__(self, latents, t, **kwargs):
            self.kwargs = kwargs
            return latents

    for name, spec in R.HINT_CASES.items():
        unet = FakeUNet()
        with torch.no_grad():
            wrapped = UC.UNetWithT2I(unet, [FakeHint(*h) for h in spec])
        out[f"cond.{name}.spec"] = np.array(json.dumps(spec))
        if wrapped.standard_states is not None:
            for side in ("u", "g", "f"):
                for i, t in enumerate(wrapped.standard_states[side]):
                    out[f"cond.{name}.{side}{i}"] = t.numpy()
        if wrapped.style_states is not None:
            out[f"cond.{name}.style"] = wrapped.style_states.numpy()
            n = wrapped.style_states.shape[0]
            if wrapped.standard_states is None:
                wrapped.standard_dim0 = n                                   # (read by __call__ before it looks at cfg_meta)
            for side in ("u", "g", "f"):
                ctx = R.hint_context(n * (2 if side == "f" else 1), fcfg["width"])
                wrapped(torch.zeros(1), 0, encoder_hidden_states=ctx, cfg_meta=side)
                out[f"cond.{name}.ctx_{side}"] = unet.kwargs["encoder_hidden_states"].numpy()
    # UnifiedPipelineHint_T2i.style_call over a fake vision_model that returns seeded hidden states (tests/t2i_seq_ref.FakeVision) and
    # the reference's own StyleAdapter with the weights above, at clip_layer final / penultimate / 3.  Three things the build container
    # cannot execute are filled in, and stay unpinned: images.rescale runs on the resize_right package (stubbed here), so the
    # repository's restatement of it is installed in its place; torchvision's Normalize is a stub, so (x - mean) / std stands in; and
    # diffusers' get_parameter_dtype is a stub, so the dtype of the model's first parameter stands in.
    from types import SimpleNamespace
    from gyre.pipeline import unified_pipeline as UP
    from gyre_amd import images as gimages
    UP.images.rescale = gimages.rescale
    UP.modeling_utils.get_parameter_dtype = lambda m: next(m.parameters()).dtype          # (diffusers is a stub here as well)
    vision = R.FakeVision(scfg["width"])
    fe = SimpleNamespace(**R.STYLE_EXTRACTOR)
    image = R.style_hint_image()
    for layer in R.STYLE_LAYERS:
        h = object.__new__(UP.UnifiedPipelineHint_T2i)
        h.model, h.image, h.mask, h.weight = style, image, None, R.STYLE_HINT_WEIGHT
        h.soft_injection, h.cfg_only, h.fuser, h.clip_layer, h.type = False, False, None, layer, "style"
        h.clip_model, h.feature_extractor = SimpleNamespace(vision_model=vision), fe
        h.style_setup()
        mean, std = torch.tensor(fe.image_mean).view(1, 3, 1, 1), torch.tensor(fe.image_std).view(1, 3, 1, 1)
        h.normalize = lambda x: (x - mean) / std
        with torch.no_grad():
            out[f"stylehint.{layer}.out"] = h().numpy()
        out[f"stylehint.{layer}.seen"] = vision.seen.numpy()
        out[f"stylehint.{layer}.all_layers"] = np.array(vision.asked_all)
    path = os.path.join(HERE, "t2i_seq_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
