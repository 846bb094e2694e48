"""Launch count and workspace size of one forward of each image-model family (-m gpu), pinned, and the order of its weight keys.  The
eight graphs share their base, the window transformers their trunk, and all their handle shell (csrc/model_upscaler.h); a change to any
of them shows up here as a deliberate edit of a number.  The numbers of the three upscalers were recorded from the commit before their
graphs were moved onto the shared trunk ("The upscaler graphs share one trunk"), those of the five hinter graphs from the
commit before all eight were moved onto the shared base ("The image graphs share one base"); they are the same in both
storage flavours.  They are those of the FIRST forward of a fresh module: it includes the launches that fill the derived weight copies
(SwinIR's expanded position bias per block, the chunk-ordered weights of RRDB's fused convolutions).

The key order - the index order of gyre_<kind>_param_key, which is the order of the store's allocations - is the state-dict order of
weights.<kind>_param_shapes less the buffers, as it was at both of those commits; the sha1 of the joined list recorded there is held too."""
import ctypes as C
import hashlib

import pytest
import torch

import hat_ref
import hed_ref
import lineart_ref
import mlsd_ref
import swinb_ref
import swinir_ref
import uniformer_ref
from gyre_amd import config as gcfg, weights
from gyre_amd.hinters import GyreHipDrawingGenerator, GyreHipHED, GyreHipMLSD, GyreHipSwinB, GyreHipUniFormer
from gyre_amd.upscaler import GyreHipHAT, GyreHipRRDBNet, GyreHipSwinIR
from gpu_util import DEV

pytestmark = pytest.mark.gpu
_rand = lambda shape: torch.rand(shape, generator=torch.Generator().manual_seed(0))
_tracked = lambda key: key.endswith("num_batches_tracked")


# each: (module, weights, image, the family's key shapes, which of them are buffers)
def _swinir():
    cfg, sd, _ = swinir_ref.model_case("tiny")          # tiny_swinir()
    return GyreHipSwinIR(cfg), sd, _rand((1, 3, 16, 24)), weights.swinir_param_shapes(cfg), weights.swinir_is_buffer


def _hat():
    cfg, sd, _ = hat_ref.model_case("tiny")             # tiny_hat()
    return GyreHipHAT(cfg), sd, _rand((1, 3, 32, 48)), weights.hat_param_shapes(cfg), weights.hat_is_buffer


def _rrdb():
    cfg = gcfg.tiny_rrdb()
    shapes = weights.rrdb_param_shapes(cfg)
    return GyreHipRRDBNet(cfg), weights.synthetic_state_dict(shapes), _rand((2, 3, 24, 20)), shapes, None


def _lineart():
    cfg, sd, x = lineart_ref.model_case("tiny")         # 1 x 3 x 8 x 12, one residual block
    return GyreHipDrawingGenerator(3, 1, cfg.n_residual_blocks, cfg.sigmoid), sd, x, weights.lineart_param_shapes(cfg), None


def _hed():
    sd, x = hed_ref.model_case("1x1")                   # 2 x 3 x 1 x 1: stage 1 works at 69 x 69
    return GyreHipHED(), sd, x, weights.hed_param_shapes(), None


def _mlsd():
    sd, x = mlsd_ref.model_case("16x16")                # 1 x 4 x 16 x 16
    return GyreHipMLSD(), sd, x, weights.mlsd_param_shapes(), _tracked


def _swinb():
    m = GyreHipSwinB(**swinb_ref.TINY)
    shapes = weights.swinb_param_shapes(m.config)       # 50 x 70: no multiple of 4 or of 48, so the padding path runs
    return m, swinb_ref.seeded_state_dict(shapes), _rand((1, 3, 50, 70)), shapes, weights.swinb_is_buffer


def _uniformer():
    m = GyreHipUniFormer(**uniformer_ref.TINY)
    shapes = weights.uniformer_param_shapes(m.config)
    return m, uniformer_ref.seeded_state_dict(shapes), _rand((1, 3, 64, 96)), shapes, _tracked


# family: (case, launches of the first forward, workspace bytes, number of keys, sha1 of the keys joined by newlines)
PINS = {"swinir": (_swinir, 53, 1818624, 74, "7fa581afa356036a029e9548beaf2425df804a85"),
        "hat": (_hat, 91, 8060928, 130, "ce77b0540ab753abbe9dfededc470ca46b0d942c"),
        "rrdb": (_rrdb, 76, 4423680, 72, "8c30d27a40c26f8b07a29ae03de2d3a849bcfe26"),
        "lineart": (_lineart, 34, 75264, 16, "52304f19a0231e381ef932ae84709f5ec46c63a8"),
        "hed": (_hed, 44, 3531776, 38, "f2f43349fad0394a45d336b01e74d005edccd774"),
        "mlsd": (_mlsd, 75, 45056, 305, "125ad304eb6610448ae31ace349befe4a082dba2"),
        "swinb": (_swinb, 80, 165376, 125, "94da1ecc61a002503c9526bdadc8970dc90c8287"),
        "uniformer": (_uniformer, 65, 393216, 126, "6364264ccabdf21ac229cb23361122228ee0c235")}


@pytest.mark.parametrize("sdt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("family", list(PINS))
def test_forward_launch_count_and_workspace(family, sdt):
    make, launches, workspace = PINS[family][:3]
    m, sd, x = make()[:3]
    m.load_state_dict(sd, strict=False)                 # (the buffers of the reference's modules are not in the synthetic weights)
    m = m.to(sdt).to(DEV)
    out = m(x.to(DEV))
    torch.cuda.synchronize()
    shape = tuple(x.shape)
    got = (int(m._L().gyre_last_launch_count()), m.workspace_bytes(shape[0], shape[2], shape[3], torch.device(DEV)))
    outs = out if isinstance(out, (list, tuple)) else [out]
    print(f"[pins] {family} {sdt}: {got[0]} launches, {got[1]} workspace bytes, output {[tuple(o.shape) for o in outs]}")
    assert got == (launches, workspace)


@pytest.mark.parametrize("family", list(PINS))
def test_param_key_order(family):
    make, _, _, count, digest = PINS[family]
    m, _, _, shapes, is_buffer = make()
    m = m.to(DEV)
    h, L = C.c_void_p(m._sync(torch.device(DEV))), m._L()
    n = getattr(L, f"gyre_{family}_num_params")(h)
    keys = [getattr(L, f"gyre_{family}_param_key")(h, i).decode() for i in range(n)]
    print(f"[pins] {family}: {n} keys, sha1 {hashlib.sha1(chr(10).join(keys).encode()).hexdigest()}")
    assert keys == [k for k in shapes if not (is_buffer and is_buffer(k))]
    assert (n, hashlib.sha1("\n".join(keys).encode()).hexdigest()) == (count, digest)
