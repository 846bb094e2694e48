"""Where the model runtime takes the four-parity upsampler form (gyre_debug_ups4_plan: the rule Exec::conv3 itself asks).  No GPU.

The form needs the planner to hand the K = 4 Cin problem the pipelined 256x320 tile (config 24): >= 20 K steps on >= 160 tiles, or
the split-K form from K >= 5000.  Tile counts below are 4 ceil(B Hi Wi / 256) ceil(N / 320)."""
import ctypes as C

import pytest

from gyre_amd import _lib

UNIT = 10            # GroupNorm statistics unit of SD1.x / SDXL: gcd of block_out_channels / 32
NO_UPS4, UPS4_ALL = 1 << 29, 1 << 30


def query(L, B, Hi, Wi, Cin, N, Hup=0, Wup=0, tiling=0, unit=UNIT):
    out = (C.c_int32 * 4)()
    assert L.gyre_debug_ups4_plan(B, Hi, Wi, Cin, N, Hup, Wup, tiling, unit, out) == 0, L.gyre_last_error()
    return tuple(out)


@pytest.fixture(params=[_lib.BF16, _lib.F16], ids=["bf16", "f16"])
def L(request):
    lib = _lib.lib(request.param)
    old = lib.gyre_debug_gemm_ablation(0)
    inv = lib.gyre_set_batch_invariant(0)
    yield lib
    lib.gyre_debug_gemm_ablation(old)
    lib.gyre_set_batch_invariant(inv)


def test_sd15_upsamplers_at_batch_16(L):
    # 32x32 -> 64x64, 640: 256 x 2 = 512 tiles, 40 K steps; 16x16 -> 32x32, 1280: 64 x 4 = 256 tiles, 80 steps; both unsplit with the
    # statistics of whole 256-pixel blocks.  8x8 -> 16x16, 1280: 16 x 4 = 64 tiles, K = 5120: 4 slices of 20 steps; its statistics
    # come from the reduction kernel in 16-row blocks
    assert query(L, 16, 32, 32, 640, 640) == (1, 24, 1, 256)
    assert query(L, 16, 16, 16, 1280, 1280) == (1, 24, 1, 256)
    assert query(L, 16, 8, 8, 1280, 1280) == (1, 24, 4, 16)


def test_768px_and_sdxl_upsamplers(L):
    # SDXL at 128x128 latents, batch 4 (2 images with CFG): 64x64 -> 128x128, 640: 256 x 2 = 512 tiles; 32x32 -> 64x64, 1280: 64 x 4 = 256
    assert query(L, 4, 64, 64, 640, 640) == (1, 24, 1, 256)
    assert query(L, 4, 32, 32, 1280, 1280) == (1, 24, 1, 256)
    # SD1.5 at 96x96 latents: 24x24 -> 48x48, 1280 at batch 4: 36 x 4 = 144 tiles, the planner's 128 - 159-tile rule for long convs
    # (80 K steps); 576 source pixels per sample are no whole 256-pixel blocks: no producer statistics
    assert query(L, 4, 24, 24, 1280, 1280) == (1, 24, 1, 0)
    # ... while 48x48 -> 96x96, 640 at batch 8 stays where the planner has the nine-tap problem too: 288 x 2 = 576 tiles of 256x320 are
    # 2.25 rounds of the 256 CUs (efficiency 0.75), the 128x160 tile fills them - the form needs config 24, so nine taps are kept
    assert query(L, 8, 48, 48, 640, 640)[0] == 0
    # the deepest 768-px level (12x12 -> 24x24: 20 x 4 = 80 tiles at batch 8) can only come in K slices, if at all
    take, cfg, splits, _ = query(L, 8, 12, 12, 1280, 1280)
    assert (take, cfg) in ((0, 0), (1, 24)) and (not take or splits > 1)


def test_refusals(L):
    assert query(L, 16, 32, 32, 640, 640, Hup=63, Wup=63)[0] == 0            # the 2H-1 crop of forward_upsample_size
    assert query(L, 16, 32, 32, 640, 640, Hup=64, Wup=63)[0] == 0
    assert query(L, 16, 32, 32, 608, 640)[0] == 0                            # Cin % 64
    for tiling in (1, 2, 3):
        assert query(L, 16, 32, 32, 640, 640, tiling=tiling)[0] == 0
    for shape in ((2, 32, 32, 640, 640), (2, 16, 16, 1280, 1280), (2, 8, 8, 1280, 1280)):      # batch 2: 64 / 32 / 8 tiles
        assert query(L, *shape)[0] == 0, shape
    L.gyre_set_batch_invariant(16)
    assert query(L, 16, 32, 32, 640, 640)[0] == 0
    L.gyre_set_batch_invariant(0)
    L.gyre_debug_gemm_ablation(NO_UPS4)
    assert query(L, 16, 32, 32, 640, 640)[0] == 0
    L.gyre_debug_gemm_ablation(NO_UPS4 | UPS4_ALL)                           # bit 29 wins
    assert query(L, 16, 32, 32, 640, 640)[0] == 0


def test_bit_30_accepts_the_small_test_shapes(L):
    shapes = ((2, 8, 8, 64, 40), (1, 16, 16, 128, 328), (3, 16, 8, 64, 64), (2, 8, 8, 320, 64), (3, 8, 8, 64, 64), (3, 4, 4, 128, 128))
    for s in shapes:
        assert query(L, *s, unit=8)[0] == 0, s                               # far too few tiles for the rule
    L.gyre_debug_gemm_ablation(UPS4_ALL)
    for s in shapes:
        take, cfg, splits, rows = query(L, *s, unit=8)
        # statistics only for whole 256-pixel blocks per sample and parity
        assert (take, cfg, splits) == (1, 24, 1) and rows == (256 if (s[1] * s[2]) % 256 == 0 else 0), (s, take, cfg, splits, rows)
    assert query(L, 1, 16, 16, 128, 328, unit=0)[3] == 0
    assert query(L, 2, 8, 8, 72, 64, unit=8)[0] == 0                         # the kernel itself needs whole 64-channel chunks
    assert query(L, 2, 8, 8, 64, 64, Hup=15, Wup=16, unit=8)[0] == 0


def test_bad_arguments(L):
    out = (C.c_int32 * 4)()
    assert L.gyre_debug_ups4_plan(0, 8, 8, 64, 64, 0, 0, 0, 0, out) == -1
    assert L.gyre_debug_ups4_plan(2, 8, 8, 64, 64, 14, 0, 0, 0, out) == -1
    assert L.gyre_debug_ups4_plan(2, 8, 8, 64, 64, 0, 0, 0, 0, None) == -1
