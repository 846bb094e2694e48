"""Build-container probe: the REFERENCE's own line-art generator and pipeline (gyre/pipeline/hinters/models/informative_drawings.py
and gyre/pipeline/hinters/informative_drawing_pipeline.py, loaded from /root/reference by file path) against tests/lineart_ref.py and
gyre_amd on the same synthetic weights.

The model file imports torch.nn alone.  The pipeline file imports ``kornia``, ``torchvision`` and ``diffusers.models.modeling_utils``,
of which it uses the two parameter queries of the last; they are satisfied by stand-in modules.  ``gyre.images`` is the reference's
own file (its ``normalise_tensor`` is torch alone; what else that file imports and this machine lacks is stood in for as well) - the
host steps under test are the reference's own code.

reference_outputs() is also what tests/golden/make_lineart_golden.py stores.  Prints one JSON object.  Run by
tests/test_reference_lineart.py; nothing here ships."""
import importlib.util
import json
import os
import sys
import types

import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lineart_ref as R  # noqa: E402
from gyre_amd import config as gcfg, hinters as HN, weights  # noqa: E402

# (model case of lineart_ref.MODEL_CASES, image shape): the golden vectors - one plain and one odd size
# what gyre/images.py imports at module level and this machine may lack; normalise_tensor, the one function under test, uses torch alone
IMAGES_STAND_INS = ("cv2", "tqdm")
GOLDEN_CASES = [("tiny", (1, 3, 8, 12)), ("odd", (1, 3, 13, 18))]


def stand_in(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__["__getattr__"] = lambda attr: Anything()           # whatever else the importer looks up at import time
    m.__dict__.update(attrs)
    m.__path__ = []
    sys.modules[name] = m
    parent, _, leaf = name.rpartition(".")
    if parent and parent in sys.modules:
        setattr(sys.modules[parent], leaf, m)
    return m


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class Anything:
    """answers every attribute with itself: default arguments that name an interpolation method at import time"""

    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        return self

    def __iter__(self):
        return iter(())

    def __getitem__(self, key):
        return self

    def __call__(self, *a, **k):
        return a[0] if len(a) == 1 and not k and callable(a[0]) else self      # (as a decorator: the identity)


def reference_model():
    return load("gyre/pipeline/hinters/models/informative_drawings.py", "ref_informative_drawings")


def reference_outputs():
    """{case: output of the reference's own DrawingGenerator on the case's synthetic weights and image}"""
    arch = reference_model()
    out = {}
    for name, shape in GOLDEN_CASES:
        cfg, sd, x = R.model_case(name)
        assert tuple(x.shape) == shape
        net = arch.DrawingGenerator(cfg.input_nc, cfg.output_nc, cfg.n_residual_blocks, cfg.sigmoid).eval()
        net.load_state_dict(sd, strict=True)
        with torch.no_grad():
            out[name] = net(x)
    return out


def main():
    arch = reference_model()
    res = dict(shapes={}, forward={}, strict_load={}, pipeline={})
    for blocks in (1, 3, 9):
        ref_sd = arch.DrawingGenerator(3, 1, blocks).state_dict()
        mine = weights.lineart_param_shapes(gcfg.lineart_config(3, 1, blocks))
        res["shapes"][str(blocks)] = dict(n=len(ref_sd), same=({k: tuple(v.shape) for k, v in ref_sd.items()} == dict(mine)),
                                          same_order=list(ref_sd) == list(mine))
    for name in ("tiny", "shipped", "odd"):
        cfg, sd, x = R.model_case(name)
        net = arch.DrawingGenerator(cfg.input_nc, cfg.output_nc, cfg.n_residual_blocks, cfg.sigmoid).eval()
        net.load_state_dict(sd, strict=True)
        with torch.no_grad():
            ref = net(x)
            mine = R.net(sd, cfg, x)
        res["forward"][name] = dict(shape=list(ref.shape), equal=bool(torch.equal(ref, mine)), max_abs=float((ref - mine).abs().max()),
                                    ref_absmax=float(ref.abs().max()))
    # a strict load of the reference's own state dict into the native shell
    ref_net = arch.DrawingGenerator(3, 1, 3)
    shell = HN.GyreHipDrawingGenerator(3, 1, 3)
    r = shell.load_state_dict(ref_net.state_dict(), strict=True)
    res["strict_load"] = dict(missing=list(r.missing_keys), unexpected=list(r.unexpected_keys),
                              same=all(torch.equal(v, shell.state_dict()[k]) for k, v in ref_net.state_dict().items()))
    # the pipeline's host steps: both pipelines over the SAME host module (the reference's own generator)
    stand_in("kornia")
    stand_in("torchvision")
    stand_in("diffusers")
    stand_in("diffusers.models")
    stand_in("diffusers.models.modeling_utils", get_parameter_device=lambda m: next(m.parameters()).device,
             get_parameter_dtype=lambda m: next(m.parameters()).dtype)
    stand_in("gyre")
    for dep in IMAGES_STAND_INS:
        try:
            __import__(dep)
        except ImportError:
            stand_in(dep)
    stand_in("gyre.images_shuffle", ContentShuffleDetector=Anything)
    stand_in("gyre.match_histograms", match_histograms=None)
    stand_in("gyre.resize_right", interp_methods=Anything(), resize=None)
    try:
        load("gyre/images.py", "gyre.images")
        sys.modules["gyre"].images = sys.modules["gyre.images"]
        ref_pipe_mod = load("gyre/pipeline/hinters/informative_drawing_pipeline.py", "ref_informative_drawing_pipeline")
    except Exception as e:                                                          # a dependency of gyre/images.py that is not installed here
        res["pipeline"] = dict(error=f"{type(e).__name__}: {e}")
        print("PROBE_JSON " + json.dumps(res))
        return
    cfg, sd, _ = R.model_case("tiny")
    host = arch.DrawingGenerator(3, 1, 1, False).eval()
    host.load_state_dict(sd)
    ref_pipe, my_pipe = ref_pipe_mod.InformativeDrawingPipeline(host), HN.GyreInformativeDrawingPipeline(host)
    g = torch.Generator().manual_seed(4)
    for label, x in (("1ch", torch.rand((2, 1, 8, 12), generator=g)), ("3ch", torch.rand((1, 3, 8, 12), generator=g)),
                     ("4ch", torch.rand((1, 4, 8, 12), generator=g)), ("3dim", torch.rand((3, 8, 12), generator=g)),
                     ("f64", torch.rand((1, 3, 8, 12), generator=g).double())):
        a, b = ref_pipe(x), my_pipe(x)
        res["pipeline"][label] = dict(equal=bool(torch.equal(a, b)), same_dtype=a.dtype == b.dtype, shape=list(a.shape))
    res["pipeline"]["modules"] = [n for n, _ in my_pipe.pipeline_modules()] == [n for n, _ in ref_pipe.pipeline_modules()]
    print("PROBE_JSON " + json.dumps(res))


if __name__ == "__main__":
    main()
