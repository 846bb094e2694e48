"""Dev tool: what the bind slots of the native ControlNet are worth under hires fix (profiles/ctrl_slots_time.json).  One SD1.5-shaped
control model serves the two leaves of a 768 x 768 request at model batch 2 (one image with parallel CFG, or two without) and at
model batch 4 (two images with parallel CFG): the natural-size leaf
(64 x 64 latents, 512 x 512 hint image) and the full-size leaf (96 x 96 latents, 768 x 768 hint image) alternate on it every step.

  slots     each leaf bound once on a slot of its own; a step is forward(slot 0) + forward(slot 1)
  rebind    what hints.REBIND_EVERY_CALL does: a step is bind + forward for the one leaf, bind + forward for the other, all on slot 0
  masked    `slots` with a residual mask pyramid on both binds (the masked hand-off kernel instead of the plain one)

One process, HIP events around ITERS steps, ROUNDS alternating rounds, median (min - max); the clocks rocm-smi reports are recorded
after a warm-up and at the end.  These are calls of the control model in a loop, not steps of a whole pipeline.  `python tools/ctrl_slots_time.py [out.json]`.  Synthetic N(0, 1/fan_in) weights, bf16 storage."""
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gyre_amd import config as gcfg
from gyre_amd.controlnet import GyreHipControlNet

dev = "cuda:0"
ROUNDS = int(os.environ.get("ROUNDS", "7"))
ITERS = int(os.environ.get("ITERS", "10"))


def fill(m):
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if p.ndim > 1:
                p.copy_(torch.randn(p.shape, device=dev, generator=g, dtype=torch.float32) / p[0].numel() ** 0.5)
            elif k.endswith("weight"):
                p.fill_(1.0)
            else:
                p.zero_()
    m._invalidate()
    return m


def clocks():
    try:
        return subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout.strip().splitlines()
    except Exception as e:                   # the figures stand without it; say so in the record
        return [f"rocm-smi not read: {e}"]


def timeit(fn, iters):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


ctrl = fill(GyreHipControlNet(gcfg.sd15_controlnet()).to(torch.bfloat16).to(dev))


def measure(B):
    ctx = torch.randn(B, 77, 768, device=dev)
    t = torch.full((B,), 500, device=dev)
    leaves = []
    for lat in (64, 96):
        x = torch.randn(B, 4, lat, lat, device=dev)
        img = torch.rand(1, 3, 8 * lat, 8 * lat, device=dev)
        outs = ctrl.new_outputs(B, lat, lat, dev)
        masks = [torch.rand(1, 1, rh, rw, device=dev) for _, rh, rw in ctrl.residual_shapes(lat, lat)]
        leaves.append((x, img, outs, masks))

    def bind_slots(masked):
        for slot, (x, img, outs, masks) in enumerate(leaves):
            ctrl.bind(img, ctx, slot=slot, masks=masks if masked else None)

    def step_slots():
        for slot, (x, img, outs, masks) in enumerate(leaves):
            ctrl(x, t, out=outs, slot=slot)

    def step_rebind():
        for x, img, outs, masks in leaves:
            ctrl.bind(img, ctx)
            ctrl(x, t, out=outs)

    bind_slots(False)
    step_slots()
    want = [[o.clone() for o in outs] for _, _, outs, _ in leaves]
    step_rebind()
    same = all(torch.equal(a, b) for w, (_, _, outs, _) in zip(want, leaves) for a, b in zip(w, outs))
    for _ in range(3):                       # warm-up of every shape the timed window uses
        bind_slots(False)                    # (step_rebind leaves slot 0 on the full-size image)
        timeit(step_slots, ITERS); timeit(step_rebind, ITERS)
    before = clocks()
    ms = {"slots": [], "rebind": [], "masked": []}
    for _ in range(ROUNDS):
        bind_slots(False)
        ms["slots"].append(timeit(step_slots, ITERS))
        ms["rebind"].append(timeit(step_rebind, ITERS))
        bind_slots(True)
        ms["masked"].append(timeit(step_slots, ITERS))
    bind_ms = {str(8 * lat): timeit(lambda img=img: ctrl.bind(img, ctx), 5) for lat, (_, img, _, _) in zip((64, 96), leaves)}
    row = {"model_batch": B, "results_bit_identical": bool(same), "bind_ms_by_image_size": bind_ms,
           "step_ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()},
           "clocks_after_warmup": before, "clocks_at_end": clocks()}
    row["rebind_over_slots"] = row["step_ms"]["rebind"]["median"] / row["step_ms"]["slots"]["median"]
    return row


props = torch.cuda.get_device_properties(0)
result = {"what": "ms per pair of control-model calls (natural-size leaf + full-size leaf of a 768x768 hires-fix request), one SD1.5-shaped "
                  "control model, calls in a loop - not whole pipeline steps",
          "rounds": ROUNDS, "steps_per_round": ITERS, "storage": "bf16", "device": props.name, "arch": getattr(props, "gcnArchName", ""),
          "compute_units": props.multi_processor_count, "batches": [measure(2), measure(4)]}
print(json.dumps(result, indent=1))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(result, f, indent=1)
