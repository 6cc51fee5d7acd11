"""The entry-point code of bloom.hip that no other test calls directly: what each bloom entry point refuses, and under which name,
and the rectangle forms of the prefilter against the whole-image call.  The expected messages are the ones the C ABI has given
since these entry points were added (include/pbr_hip.h documents the refusals); a refused call enqueues nothing."""
import numpy as np
import pytest
import torch

from direct12pbrrenderer_amd import synth
from direct12pbrrenderer_amd.api import PbrError

pytestmark = pytest.mark.gpu

POISON = np.float16(777.0)


def dev_half(ctx, arr):
    return ctx.upload(np.ascontiguousarray(arr, dtype=np.float16).view(np.uint16)).view(torch.float16)


def bits(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


@pytest.fixture(scope="module")
def buf(ctx):
    """Device memory for the refused calls: 256 x 256 half4 texels per buffer, more than any size claimed below, so that a call
    which is wrongly accepted still stays inside its buffers."""
    return [ctx.zeros((256 * 256, 4), torch.float16) for _ in range(4)] + [ctx.zeros((256,), torch.int32)]


def _bad_calls(ctx, b):
    hdr, a, c, out, hist = b
    good = (8, 8, 16, 8)   # a rectangle inside the 80 x 36 half-res image of 160 x 72
    return {
        "bloom 8x8": (lambda: ctx.bloom(hdr, 8, 8, 8, a, c), "status -1: pbr_bloom: image too small for 5 mips"),
        # pbr_bloom_histogram checks its sizes in the code it shares with pbr_bloom, under that name
        "bloom_histogram 8x8": (lambda: ctx.bloom_histogram(hdr, 8, 8, 8, a, c, (0, 0, 8, 8), hist),
                                "status -1: pbr_bloom: image too small for 5 mips"),
        "bloom_histogram rect past the image": (lambda: ctx.bloom_histogram(hdr, 64, 64, 64, a, c, (1, 0, 64, 64), hist),
                                                "status -1: pbr_bloom_histogram: rect outside the image"),
        "bloom_prefilter pitch < w": (lambda: ctx.bloom_prefilter(hdr, 64, 64, 63, out), "status -1: pbr_bloom_prefilter: bad size"),
        "bloom_prefilter_rect rect past the half-res image": (lambda: ctx.bloom_prefilter_rect(hdr, 160, 72, 160, out, 96, 0, 0, (70, 8, 11, 8)),
                                                              "status -1: pbr_bloom_prefilter_rect: rect outside the half-res image"),
        "bloom_prefilter_rect out_pitch too small": (lambda: ctx.bloom_prefilter_rect(hdr, 160, 72, 160, out, 30, 7, 0, good),
                                                     "status -1: pbr_bloom_prefilter_rect: rect does not fit the output pitch"),
        "bloom_prefilter_rects 0 rectangles": (lambda: ctx.bloom_prefilter_rects(hdr, 160, 72, 160, out, 96, 0, 0, []),
                                               "status -1: pbr_bloom_prefilter_rects: null pointer / 1 .. 5 rectangles"),
        "bloom_prefilter_rects 6 rectangles": (lambda: ctx.bloom_prefilter_rects(hdr, 160, 72, 160, out, 96, 0, 0, [good] * 6),
                                               "status -1: pbr_bloom_prefilter_rects: null pointer / 1 .. 5 rectangles"),
        "bloom_prefilter_rects one bad rectangle among good ones": (
            lambda: ctx.bloom_prefilter_rects(hdr, 160, 72, 160, out, 96, 0, 0, [good, (8, 30, 16, 7), good]),
            "status -1: pbr_bloom_prefilter_rects: rectangle outside the half-res image / the output pitch"),
        "bloom_tiled merge_rect outside hdr_rect": (lambda: ctx.bloom_tiled(hdr, 64, (16, 16, 64, 64), 160, 96, a, c, (15, 16, 64, 64), hist),
                                                    "status -1: pbr_bloom_tiled: merge_rect outside hdr_rect"),
        "bloom_tiled odd extended size": (lambda: ctx.bloom_tiled(hdr, 64, (16, 16, 64, 64), 161, 96, a, c, (16, 16, 64, 64), hist),
                                          "status -4: pbr_bloom_tiled: the extended tile must be even and <= 8192 on a side"),
        "bloom_up_level out not twice lower": (lambda: ctx.bloom_up_level(a, c, 40, 18, out, 80, 38),
                                               "status -1: pbr_bloom_up_level: out must be exactly twice lower, even, <= 8192"),
        "bloom_up_level out aliases an input": (lambda: ctx.bloom_up_level(a, c, 40, 18, a, 80, 36),
                                                "status -1: pbr_bloom_up_level: null pointer / out aliases an input"),
    }


def test_refusals_keep_their_cases_and_their_names(ctx, buf):
    before = [bits(t).copy() for t in buf]
    for what, (call, message) in _bad_calls(ctx, buf).items():
        with pytest.raises(PbrError) as e:
            call()
        print(what, "->", e.value)
        assert str(e.value) == message, what
    ctx.sync()
    for t, b in zip(buf, before):   # nothing was enqueued
        assert np.array_equal(bits(t), b)


RECT = (3, 5, 70, 20)                                          # straddles a 64 x 16 tile edge of both prefilter kernels
BANDS = [(3, 5, 70, 7), (3, 12, 70, 6), (3, 18, 70, 7)]        # the same texels in three bands
OUT_PITCH, OUT_ROWS, OUT_X, OUT_Y = 96, 48, 7, 4


@pytest.fixture(scope="module", params=[(160, 72), (151, 86)], ids=["160x72-shared-sample", "151x86-staged"])
def whole(ctx, request):
    """(w, h, the image on the device, bloom_prefilter of the whole image).  160 x 72: both sides even, so the shared-sample kernel
    runs on the 80 x 36 half-res image; 151 x 86: the odd width selects the staged kernel (75 x 43)."""
    w, h = request.param
    hdr = dev_half(ctx, synth.hdr_noise_image(w, h, seed=11))
    out = ctx.zeros((h // 2, w // 2, 4), torch.float16)
    ctx.bloom_prefilter(hdr, w, h, w, out)
    return w, h, hdr, bits(out)


def _expected_window(full):
    x, y, rw, rh = RECT
    want = np.full((OUT_ROWS, OUT_PITCH, 4), POISON, dtype=np.float16).view(np.uint16)
    want[OUT_Y + y: OUT_Y + y + rh, OUT_X + x: OUT_X + x + rw] = full[y: y + rh, x: x + rw]
    return want


def _poisoned(ctx):
    return dev_half(ctx, np.full((OUT_ROWS, OUT_PITCH, 4), POISON, dtype=np.float16))


def test_prefilter_rect_writes_exactly_the_window_of_the_whole(ctx, whole):
    w, h, hdr, full = whole
    dst = _poisoned(ctx)
    ctx.bloom_prefilter_rect(hdr, w, h, w, dst, OUT_PITCH, OUT_X, OUT_Y, RECT)
    assert np.array_equal(bits(dst), _expected_window(full))


def test_prefilter_rects_in_three_bands_give_the_same_bits(ctx, whole):
    w, h, hdr, full = whole
    dst = _poisoned(ctx)
    ctx.bloom_prefilter_rects(hdr, w, h, w, dst, OUT_PITCH, OUT_X, OUT_Y, BANDS)
    assert np.array_equal(bits(dst), _expected_window(full))
