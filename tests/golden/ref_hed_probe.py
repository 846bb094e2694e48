"""Build-container probe: the REFERENCE's own HED and HedPipeline (gyre/pipeline/hinters/models/hed.py and
gyre/pipeline/hinters/hed_pipeline.py, loaded from /root/reference by file path) against tests/hed_ref.py and gyre_amd on the same
seeded weights.

The model file imports numpy and torch alone.  The pipeline file imports ``kornia``, ``torchvision`` and
``diffusers.models.modeling_utils``, of which it uses the two parameter queries of the last; they are satisfied by the stand-in modules
of ref_lineart_probe.py.  ``gyre.images`` is the reference's own file - the host steps under test (``normalise_tensor``,
``normalise_range``) are the reference's own code.

reference_geometry() and reference_maps() are also what tests/golden/make_hed_golden.py stores.  Prints one JSON object.  Run by
tests/test_reference_hed.py; nothing here ships."""
import json
import os
import sys

import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_lineart_probe as LP  # noqa: E402  (the stand-in machinery; it puts the repository and tests/ on the path)
import hed_ref as R  # noqa: E402
from gyre_amd import hinters as HN, weights  # noqa: E402

SIDES = list(range(1, 81))


def reference_model():
    return LP.load("gyre/pipeline/hinters/models/hed.py", "ref_hed")


def reference_geometry(arch):
    """(stage sizes, crop offsets) per side of SIDES, read off the reference's own layers: the sizes from its convolution and pooling
    modules on a one-channel-wide strip, the offsets from its crop() on a ramp"""
    net = arch.HED()
    sizes, offsets = [], []
    for n in SIDES:
        t = torch.zeros(1, 1, n + 2 * 35 - 2, 1)                     # conv1_1: kernel 3, padding 35
        s = [t.shape[2]]
        for _ in range(4):
            t = net.maxpool(t)
            s.append(t.shape[2])
        sizes.append(s)
        o = []
        for k in range(5):
            full = s[0] if k == 0 else (s[k] - 1) * 2 ** k + 2 ** (k + 1)         # conv_transpose2d: (n - 1) stride + kernel
            ramp = torch.arange(full, dtype=torch.float32).reshape(1, 1, full, 1).expand(1, 1, full, full)
            o.append(int(arch.crop(ramp, n, n)[0, 0, 0, 0]))
        offsets.append(o)
    return sizes, offsets


def reference_maps(arch, name):
    sd, x = R.model_case(name)
    net = arch.HED().eval()
    net.load_state_dict(sd, strict=True)
    with torch.no_grad():
        return net(x)


def main():
    arch = reference_model()
    res = dict(shapes={}, geometry={}, forward={}, strict_load={}, pipeline={})
    ref_sd = arch.HED().state_dict()
    mine = weights.hed_param_shapes()
    res["shapes"] = dict(n=len(ref_sd), same=({k: tuple(v.shape) for k, v in ref_sd.items()} == dict(mine)), same_order=list(ref_sd) == list(mine))
    sizes, offsets = reference_geometry(arch)
    res["geometry"] = dict(sizes=sizes == [R.stage_sizes(n) for n in SIDES], offsets=offsets == [R.crop_offsets(n) for n in SIDES])
    for name in R.MODEL_CASES:
        ref = reference_maps(arch, name)
        sd, x = R.model_case(name)
        with torch.no_grad():
            got = R.net(sd, x)
        res["forward"][name] = dict(shape=list(ref[0].shape), n=len(ref), equal=all(bool(torch.equal(a, b)) for a, b in zip(ref, got)),
                                    max_abs=max(float((a - b).abs().max()) for a, b in zip(ref, got)))
    shell = HN.GyreHipHED()
    r = shell.load_state_dict(ref_sd, strict=True)
    res["strict_load"] = dict(missing=list(r.missing_keys), unexpected=list(r.unexpected_keys),
                              same=all(torch.equal(v, shell.state_dict()[k]) for k, v in ref_sd.items()))
    # the pipeline's host steps: both pipelines (and hed_ref's) over the SAME host module, the reference's own HED
    LP.stand_in("kornia")
    LP.stand_in("torchvision")
    LP.stand_in("diffusers")
    LP.stand_in("diffusers.models")
    LP.stand_in("diffusers.models.modeling_utils", get_parameter_device=lambda m: next(m.parameters()).device,
                get_parameter_dtype=lambda m: next(m.parameters()).dtype)
    LP.stand_in("gyre")
    for dep in LP.IMAGES_STAND_INS:
        try:
            __import__(dep)
        except ImportError:
            LP.stand_in(dep)
    LP.stand_in("gyre.images_shuffle", ContentShuffleDetector=LP.Anything)
    LP.stand_in("gyre.match_histograms", match_histograms=None)
    LP.stand_in("gyre.resize_right", interp_methods=LP.Anything(), resize=None)
    try:
        LP.load("gyre/images.py", "gyre.images")
        sys.modules["gyre"].images = sys.modules["gyre.images"]
        ref_pipe_mod = LP.load("gyre/pipeline/hinters/hed_pipeline.py", "ref_hed_pipeline")
    except Exception as e:                                                          # a dependency of gyre/images.py that is not installed here
        res["pipeline"] = dict(error=f"{type(e).__name__}: {e}")
        print("PROBE_JSON " + json.dumps(res))
        return
    host = arch.HED().eval()
    host.load_state_dict(R.model_weights())
    ref_pipe, my_pipe = ref_pipe_mod.HedPipeline(host), HN.GyreHedPipeline(host)
    g = torch.Generator().manual_seed(4)
    for label, x in (("1ch", torch.rand((2, 1, 8, 12), generator=g)), ("3ch", torch.rand((1, 3, 8, 12), generator=g)),
                     ("4ch", torch.rand((1, 4, 8, 12), generator=g)), ("3dim", torch.rand((3, 8, 12), generator=g)),
                     ("f64", torch.rand((1, 3, 8, 12), generator=g).double())):
        a, b, c = ref_pipe(x), my_pipe(x), R.pipeline(host, x)
        res["pipeline"][label] = dict(equal=bool(torch.equal(a, b)) and bool(torch.equal(a, c)), same_dtype=a.dtype == b.dtype == c.dtype,
                                      shape=list(a.shape), spread=float(a.max() - a.min()))
    res["pipeline"]["modules"] = [n for n, _ in my_pipe.pipeline_modules()] == [n for n, _ in ref_pipe.pipeline_modules()]
    print("PROBE_JSON " + json.dumps(res))


if __name__ == "__main__":
    main()
