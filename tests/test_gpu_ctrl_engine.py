"""ControlNet hints through the engine class (-m gpu): gyre_amd.engine.GyreUnifiedPipeline over the native UNet / VAE with a
GyreHipControlNet hint handler, 4 Euler steps at batch 2, against the SAME host code (GyrePipeline, ControlNetHint,
UNetWithControlnet, the CFG wrappers) over the fp32 oracle models on the CPU - the gate tests/test_gpu_t2i.py applies to its hinted
run: PSNR >= 30 dB."""
from types import SimpleNamespace

import pytest
import torch

import ctrl_ref as R
from gyre_amd import config as gcfg, weights
from gyre_amd.controlnet import GyreHipControlNet
from gyre_amd.hints import ControlNetHint
from gyre_amd.modules import set_batch_invariant
from gyre_amd.pipeline import GyrePipeline
from gyre_amd.t2i import GyreHipT2IAdapter
from gpu_util import DEV
from oracle import models_ref as M
from oracle import pipeline_ref as PR
from test_gpu_engine import build_engine, generators, wrapper_kwargs

pytestmark = pytest.mark.gpu
PRIORITY = {"balanced": dict(soft_injection=False, cfg_only=False), "prompt": dict(soft_injection=True, cfg_only=False),
            "hint": dict(soft_injection=True, cfg_only=True)}


class OracleUNet:
    def __init__(self, sd, cfg):
        self.sd, self.config = sd, cfg

    def __call__(self, latents, t, encoder_hidden_states=None, down_block_additional_residuals=None,
                 mid_block_additional_residual=None, adapter_states=None, **_):
        t = torch.as_tensor(t)
        if t.ndim == 0:
            t = t.expand(latents.shape[0])
        return SimpleNamespace(sample=M.unet_forward(self.sd, self.config, latents, t, encoder_hidden_states,
                                                     down_res=down_block_additional_residuals, mid_res=mid_block_additional_residual,
                                                     adapter_states=adapter_states))


class OracleControlNet:
    """tests/ctrl_ref.py behind the surface ControlNetHint and UNetWithControlnet use of GyreHipControlNet"""

    def __init__(self, sd, cfg):
        self.sd, self.config, self._bound = sd, cfg, None

    def bind(self, image, ctx):
        self._bound = (image.float(), ctx.float())

    def new_outputs(self, B, H, W, device, dtype=None):
        return [torch.empty((B, ch, h, w)) for ch, h, w in GyreHipControlNet.residual_shapes(self, H, W)]

    def __call__(self, x, t, *, scales, out, accumulate=False, out_batch=None, out_offset=0):
        image, ctx = self._bound
        t = torch.as_tensor(t)
        res = R.ctrl_forward(self.sd, self.config, x.float(), t, ctx, image)
        B = x.shape[0]
        for o, r, s in zip(out, res, scales):
            if not accumulate:
                o.zero_()
                o[out_offset:out_offset + B] = r * s
            else:
                o[out_offset:out_offset + B] += r * s
        return out


@pytest.fixture(scope="module")
def rig():
    from test_host_pipeline import OracleVAE
    ucfg, vcfg, ccfg, acfg = gcfg.tiny_unet(), gcfg.tiny_vae(), gcfg.tiny_controlnet(), gcfg.tiny_t2i("main")
    csd = weights.synthetic_state_dict(weights.controlnet_param_shapes(ccfg), 1)
    asd = weights.synthetic_state_dict(weights.t2i_param_shapes(acfg), 1)
    ctrl, adapter = GyreHipControlNet(ccfg), GyreHipT2IAdapter(acfg)
    ctrl.load_state_dict(csd); adapter.load_state_dict(asd)
    ctrl, adapter = ctrl.to(DEV), adapter.to(DEV)
    table = {"canny": {"canny": ctrl}, "sketch": {"sketch": adapter, "clip_model": None}}
    manager = SimpleNamespace(for_type=lambda t, default=None: table.get(t, default))
    usd, vsd, eng = build_engine(ucfg, vcfg, hintset_manager=manager)
    eng.scheduler = "euler"
    ref_pipe = GyrePipeline(OracleUNet(usd, ucfg), OracleVAE(vsd, vcfg), device="cpu")
    image = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(12))
    return SimpleNamespace(eng=eng, ref_pipe=ref_pipe, oracle_ctrl=OracleControlNet(csd, ccfg), ctrl=ctrl, image=image,
                           prompt=["a lighthouse", "a cat"], seeds=[7, 8])


def call(rig, priority="balanced", seeds=None, prompt=None, hints=None, **over):
    seeds, prompt = seeds or rig.seeds, prompt or rig.prompt
    hint = SimpleNamespace(image=rig.image, hint_type="canny", weight=0.8, priority=priority, clip_layer=None)
    args = wrapper_kwargs(prompt=prompt, negative_prompt=None, generator=generators(seeds), width=128, height=128, num_inference_steps=4,
                          hint_images=[hint] if hints is None else hints, **over)
    images, nsfw = rig.eng(**args)
    assert images.shape == (len(seeds), 3, 128, 128) and images.dtype == torch.float32 and nsfw == [False] * len(seeds)
    return images


def oracle(rig, priority, **over):
    cond, unc = rig.eng._embed(rig.prompt, None, 2, 1, True, 3)
    hint = ControlNetHint(rig.oracle_ctrl, rig.image, weight=0.8, **PRIORITY[priority])
    return rig.ref_pipe(generators=generators(rig.seeds), text_embeddings=cond.float().cpu(), uncond_embeddings=unc.float().cpu(),
                        height=128, width=128, num_inference_steps=4, sampler="euler", controlnet_hints=[hint], **over).float()


@pytest.fixture(scope="module")
def plain(rig):
    return call(rig, hints=[])


@pytest.mark.parametrize("priority", list(PRIORITY))
def test_engine_with_a_controlnet_hint_matches_the_oracle(rig, plain, priority):
    got = call(rig, priority)
    p, moved = PR.psnr(got, oracle(rig, priority)), PR.psnr(got, plain)
    print(f"[parity] engine + ControlNet hint ({priority}), euler 4 steps: PSNR {p:.1f} dB vs oracle; {moved:.1f} dB vs the un-hinted run")
    assert p >= 30.0
    assert moved < p                                                   # the hint matters
    seq = call(rig, priority, cfg_execution="sequential")
    ps = PR.psnr(seq, got)
    print(f"[parity] engine + ControlNet hint ({priority}): sequential vs parallel CFG PSNR {ps:.1f} dB")
    assert ps >= 30.0


def test_controlnet_request_is_batch_invariant(rig):
    """seeds [a, b] against [a] and [b] on the engine's own modules and embeddings: bit-identical under batch-invariant planning.
    (The embeddings are made once, at batch 2: the text encoder is host PyTorch and outside that planning.)"""
    eng = rig.eng
    cond, unc = eng._embed(rig.prompt, None, 2, 1, True, 3)
    pipe = GyrePipeline(eng.unet, eng.vae, None, device=eng.execution_device)

    def run(idx):
        hint = ControlNetHint(rig.ctrl, rig.image.to(DEV), weight=0.8, **PRIORITY["prompt"])
        return pipe(generators=generators([rig.seeds[i] for i in idx]), text_embeddings=cond[idx].contiguous(),
                    uncond_embeddings=unc[idx].contiguous(), height=128, width=128, num_inference_steps=4, sampler="euler",
                    controlnet_hints=[hint]).float().cpu()
    prev = set_batch_invariant(16)
    try:
        both = run([0, 1])
        for i in range(2):
            assert torch.equal(both[i:i + 1], run([i]))
        assert torch.equal(both, call(rig, "prompt"))                  # and it is the engine's own result
    finally:
        set_batch_invariant(prev)


def test_engine_controlnet_and_t2i_hint_in_one_request(rig, plain):
    hints = [SimpleNamespace(image=rig.image, hint_type="canny", weight=0.8, priority="hint", clip_layer=None),
             SimpleNamespace(image=rig.image, hint_type="sketch", weight=0.6, priority="prompt", clip_layer=None)]
    both = call(rig, hints=hints)
    assert bool(torch.isfinite(both).all()) and not torch.equal(both, plain)
    assert not torch.equal(both, call(rig, "hint"))
