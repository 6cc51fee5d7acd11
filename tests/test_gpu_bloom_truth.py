"""The bloom kernels (csrc/bloom.hip) under the float64 truth of tests/bloom_truth.py: every staged entry point stage by stage, the
fused up-level and the whole pyramid by interval propagation, the polyphase kernel at the smallest shapes where it can go wrong
(knobs build, child process) and at the smallest sizes that select it in the product library.  Inputs sit between poisoned guard
texels, outputs and scratch are poisoned before each call, and every call runs twice with different poison: the bits must not
change.  The bands, conditions and case sets are bloom_truth's; tests/test_bloom_truth_cpu.py holds the CPU oracle to the same
assertions.  `-s` prints the measured figures."""
import os

import numpy as np
import pytest
import torch

import bloom_truth as bt
import common

pytestmark = pytest.mark.gpu

GUARD = 64                                # texels in front of and behind every plane: 512 bytes, so the plane keeps its alignment
POISONS = (0x7E5A, 0xFBFF)                # a NaN; -65504: neither survives a band, and the two leave different traces


class Plane:
    """[h, w, 4] half texels on the device between two guards of poison.  arr None: the plane itself is poison (an output, scratch)."""

    def __init__(self, ctx, poison, arr=None, texels=None):
        n = texels if arr is None else arr.shape[0] * arr.shape[1]
        host = np.full((n + 2 * GUARD, 4), poison, dtype=np.uint16)
        if arr is not None:
            host[GUARD:GUARD + n] = np.ascontiguousarray(arr, dtype=np.float16).view(np.uint16).reshape(n, 4)
        self.n, self.poison = n, poison
        self.t = ctx.upload(host)
        self.ptr = self.t.data_ptr() + 8 * GUARD

    def bits(self):
        """the plane's texels [n, 4] uint16, after asserting that the guards were left alone"""
        host = self.t.cpu().numpy().view(np.uint16)
        assert (host[:GUARD] == self.poison).all() and (host[GUARD + self.n:] == self.poison).all(), "write outside the plane"
        return host[GUARD:GUARD + self.n].copy()

    def image(self, w, h):
        return self.bits().reshape(h, w, 4).view(np.float16)


def twice(ctx, run):
    """run(poison) -> [.., 4] half result, once per poison: the same bits both times (nothing of the poison was read, every output
    texel was written); returns them"""
    first, second = (np.ascontiguousarray(run(p)) for p in POISONS)
    ctx.sync()
    assert np.array_equal(first.view(np.uint16), second.view(np.uint16)), "the result depends on what the buffers held before"
    return first


def report(what, r):
    print(f"{what}: undecided {r['undecided']:.4%}, worst {r['worst']:.3f} of the band")


def shape_id(s):
    return "x".join(str(v) for v in s)


# ------------------------------------------------------------------------------------------------------ the staged entry points
@pytest.mark.parametrize("w,h", bt.PREFILTER_SHAPES)
@pytest.mark.parametrize("threshold,knee", bt.PREFILTER_PARAMS)
def test_prefilter(ctx, w, h, threshold, knee):
    """k_bloom_prefilter_2x at the even sizes, k_bloom_prefilter at 131 x 77"""
    for kind in bt.KINDS:
        img = bt.plane(kind, w, h, step=4)

        def run(poison):
            src, out = Plane(ctx, poison, img), Plane(ctx, poison, texels=(w >> 1) * (h >> 1))
            ctx.bloom_prefilter(src.ptr, w, h, w, out.ptr, threshold, knee)
            return out.image(w >> 1, h >> 1)
        t, m = bt.prefilter(img, threshold, knee)
        report(f"prefilter {w}x{h} ({threshold}, {knee}) {kind}", bt.check_stage(twice(ctx, run), t, bt.U * m, f"prefilter {w}x{h} {kind}"))


def _blur(ctx, call, truth, shape):
    iw, ih, ow, oh = shape
    for kind in bt.kinds_for(bt.BLUR_SHAPES.index(shape) if shape in bt.BLUR_SHAPES else 99):
        img = bt.plane(kind, iw, ih)

        def run(poison):
            src, out = Plane(ctx, poison, img), Plane(ctx, poison, texels=ow * oh)
            call(src.ptr, iw, ih, out.ptr, ow, oh)
            return out.image(ow, oh)
        t, m = truth(img, ow, oh)
        report(f"{truth.__name__} {shape} {kind}", bt.check_stage(twice(ctx, run), t, bt.band(bt.K_BLUR, m), f"{truth.__name__} {shape} {kind}"))


@pytest.mark.parametrize("shape", bt.BLUR_H_SHAPES, ids=shape_id)
def test_blur_h(ctx, shape):
    _blur(ctx, ctx.blur_h, bt.blur_h, shape)


@pytest.mark.parametrize("shape", bt.BLUR_V_SHAPES, ids=shape_id)
def test_blur_v(ctx, shape):
    _blur(ctx, ctx.blur_v, bt.blur_v, shape)


UP_PAIRS = [(lw, lh, 2 * lw, 2 * lh) for lw, lh in bt.UP_SHAPES] + [(22, 11, 45, 22)]


@pytest.mark.parametrize("shape", UP_PAIRS, ids=shape_id)
def test_upsample_add(ctx, shape):
    lw, lh, uw, uh = shape
    for kind in ("noise", "subnormal", "bright"):
        upper, lower = bt.plane(kind, uw, uh, seed=1), bt.plane(kind, lw, lh, seed=2)

        def run(poison):
            up, lo, out = Plane(ctx, poison, upper), Plane(ctx, poison, lower), Plane(ctx, poison, texels=uw * uh)
            ctx.bloom_upsample_add(up.ptr, uw, uh, lo.ptr, lw, lh, out.ptr)
            return out.image(uw, uh)
        t, m = bt.upsample_add(upper, lower)
        report(f"upsample_add {shape} {kind}", bt.check_stage(twice(ctx, run), t, bt.band(bt.K_DUAL, m), f"upsample_add {shape} {kind}"))


@pytest.mark.parametrize("kind", bt.KINDS)
def test_merge(ctx, kind):
    w, h = 67, 9
    hdr, src = bt.plane(kind, w, h, seed=3), bt.plane(kind, w, h, seed=4)

    def run(poison):
        a, b = Plane(ctx, poison, hdr), Plane(ctx, poison, src)
        ctx.bloom_merge(a.ptr, w, b.ptr, w, h)
        assert np.array_equal(b.image(w, h).view(np.uint16), src.view(np.uint16))
        return a.image(w, h)
    t, m = bt.merge(hdr, src)
    got = twice(ctx, run)
    report(f"merge {kind}", bt.check_stage(got, t, bt.band(bt.K_MERGE, m), f"merge {kind}"))
    if kind == "bright":
        assert np.isinf(got).all()


def _up_level(ctx, lower, upper, ow, oh):
    def run(poison):
        lo, out = Plane(ctx, poison, lower), Plane(ctx, poison, texels=ow * oh)
        up = Plane(ctx, poison, upper) if upper is not None else None
        ctx.bloom_up_level(up.ptr if up else None, lo.ptr, ow // 2, oh // 2, out.ptr, ow, oh)
        return out.image(ow, oh)
    return twice(ctx, run)


@pytest.mark.parametrize("dual", [True, False], ids=["dual", "single"])
@pytest.mark.parametrize("lw,lh", bt.UP_SHAPES)
def test_up_level(ctx, orc, lw, lh, dual):
    """pbr_bloom_up_level at sizes below the polyphase threshold: k_blur_hv<M_UP>, whose H result nobody sees — the two stages'
    bands propagated (bloom_truth.up_level_interval)"""
    ow, oh = 2 * lw, 2 * lh
    for kind in ("noise", "subnormal"):
        lower = bt.plane(kind, lw, lh, seed=9)
        upper = bt.plane(kind, ow, oh, seed=10) if dual else None
        got = _up_level(ctx, lower, upper, ow, oh)
        lo, hi = bt.up_level_interval(upper, lower, ow, oh)
        r = bt.check_chain(got, lo, hi, f"up_level {lw}x{lh} dual={dual} {kind}")
        staged = orc.blur_v(orc.bloom_upsample_add(upper, lower) if dual else orc.blur_h(lower, ow, oh), ow, oh)
        print(f"up_level {lw}x{lh} dual={dual} {kind}: interval at most {r['width']} wide, {r['degenerate']:.2%} degenerate, "
              f"{int((got.view(np.uint16) != staged.view(np.uint16)).sum())} values differ from the oracle's two calls")


# ------------------------------------------------------------------------------------------------------ the pyramid
CHAIN_KINDS = ("noise", "smooth", "black", "subnormal")


@pytest.mark.parametrize("w,h", bt.CHAIN_SHAPES)
def test_chain(ctx, w, h):
    """pbr_bloom and pbr_bloom_histogram: the merged frame inside the propagated interval at every texel, the same bits from both
    entry points, the histogram that of the stand-alone pass on the merged frame, both scratch chains poisoned"""
    from direct12pbrrenderer_amd.structs import bloom_chain_texels
    n = bloom_chain_texels(w, h)
    for kind in CHAIN_KINDS:
        img = bt.plane(kind, w, h)
        lo, hi = bt.chain(img)

        def run(poison, histogram=True):
            hdr, ca, cb = Plane(ctx, poison, img), Plane(ctx, poison, texels=n), Plane(ctx, poison, texels=n)
            if not histogram:
                ctx.bloom(hdr.ptr, w, h, w, ca.ptr, cb.ptr)
                ca.bits(), cb.bits()                                 # the guards behind the scratch chains
                return hdr.image(w, h)
            hist, ref = ctx.zeros((256,), torch.int32), ctx.zeros((256,), torch.int32)
            ctx.bloom_histogram(hdr.ptr, w, h, w, ca.ptr, cb.ptr, (0, 0, w, h), hist)
            ctx.lum_histogram(hdr.ptr, w, h, w, ref)
            assert np.array_equal(hist.cpu().numpy(), ref.cpu().numpy()), "the tail's histogram differs from the stand-alone pass"
            assert int(hist.sum()) == w * h
            ca.bits(), cb.bits()
            return hdr.image(w, h)
        got = twice(ctx, run)
        r = bt.check_chain(got, lo, hi, f"chain {w}x{h} {kind}")
        plain = run(POISONS[0], histogram=False)
        assert np.array_equal(plain.view(np.uint16), got.view(np.uint16)), "pbr_bloom differs from pbr_bloom_histogram"
        print(f"chain {w}x{h} {kind}: interval at most {r['width']} wide, {r['degenerate']:.2%} degenerate")


# ------------------------------------------------------------------------------------------------------ the polyphase kernel
_POLY_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
import bloom_truth as bt
import common
from oracle import binding as orc
from direct12pbrrenderer_amd.api import PbrContext
from direct12pbrrenderer_amd.structs import bloom_chain_texels
from test_gpu_bloom_truth import Plane, twice, POISONS, _up_level
ctx = PbrContext(0)
for lw, lh in bt.UP_SHAPES:
    ow, oh = 2 * lw, 2 * lh
    for dual in (True, False):
        for kind in ("noise", "subnormal"):
            lower = bt.plane(kind, lw, lh, seed=9)
            upper = bt.plane(kind, ow, oh, seed=10) if dual else None
            got = _up_level(ctx, lower, upper, ow, oh)
            lo, hi = bt.up_level_interval(upper, lower, ow, oh)
            r = bt.check_chain(got, lo, hi, "poly up_level %%dx%%d dual=%%s %%s" %% (lw, lh, dual, kind))
            staged = orc.blur_v(orc.bloom_upsample_add(upper, lower) if dual else orc.blur_h(lower, ow, oh), ow, oh)
            d = common.half_ulp_diff(got, staged)
            assert ((lo.astype(np.float64) <= staged) & (staged <= hi.astype(np.float64)))[d > 0].all()      # the oracle's value is the interval's other end
            print("poly up_level %%dx%%d dual=%%s %%s: interval at most %%d wide, %%.2f%%%% degenerate; %%d of %%d values differ from the oracle's "
                  "two calls (at most %%d ULP), both inside the interval" %% (lw, lh, dual, kind, r["width"], 100 * r["degenerate"], int((d > 0).sum()), d.size, int(d.max())))
for w, h in ((256, 128), (96, 32)):
    n = bloom_chain_texels(w, h)
    for kind in ("noise", "smooth", "subnormal"):
        img = bt.plane(kind, w, h)
        lo, hi = bt.chain(img)
        def run(poison):
            hdr, ca, cb = Plane(ctx, poison, img), Plane(ctx, poison, texels=n), Plane(ctx, poison, texels=n)
            ctx.bloom(hdr.ptr, w, h, w, ca.ptr, cb.ptr)
            ca.bits(), cb.bits()
            return hdr.image(w, h)
        got = twice(ctx, run)
        r = bt.check_chain(got, lo, hi, "poly chain %%dx%%d %%s" %% (w, h, kind))
        want = img.copy()
        orc.bloom(want)
        d = common.half_ulp_diff(got, want)
        print("poly chain %%dx%%d %%s: interval at most %%d wide, %%.2f%%%% degenerate; %%d of %%d values differ from the oracle (at most %%d ULP), "
              "all inside the interval" %% (w, h, kind, r["width"], 100 * r["degenerate"], int((d > 0).sum()), d.size, int(d.max())))
ctx.close()
print("poly truth ok")
"""


def test_polyphase_kernel_forced_on_at_small_sizes():
    """k_blur_up_poly through the knobs build (PBR_BLOOM_WIDE=1 runs it at every 2x-up level): 32 x 16 -> 64 x 32, 48 x 16 -> 96 x 32
    (below one 128-wide tile), 5 x 20 -> 10 x 40, 200 x 152 -> 400 x 304 (no multiple of 128), DUAL and not, and the whole pyramid
    at 256 x 128 and 96 x 32 — inside the truth's intervals everywhere, with the count of values that differ from the oracle"""
    root = common.ROOT
    r = common.run_child(_POLY_CHILD % (root, os.path.join(root, "tests")), {"PBR_BLOOM_WIDE": "1"}, clear=("PBR_BLOOM_WIDE",), timeout_s=300)
    print(r.stdout)
    assert r.returncode == 0 and "poly truth ok" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-4000:])


@pytest.mark.parametrize("dual", [True, False], ids=["dual", "single"])
def test_polyphase_kernel_in_the_product_library(ctx, orc, dual):
    """1024 x 400 -> 2048 x 800: 400 tiles of 128 x 32, the smallest level pbr_bloom_up_level gives to k_blur_up_poly"""
    lw, lh, ow, oh = 1024, 400, 2048, 800
    lower = bt.plane("noise", lw, lh, seed=9)
    upper = bt.plane("noise", ow, oh, seed=10) if dual else None
    got = _up_level(ctx, lower, upper, ow, oh)
    lo, hi = bt.up_level_interval(upper, lower, ow, oh)
    r = bt.check_chain(got, lo, hi, f"product poly up_level dual={dual}")
    staged = orc.blur_v(orc.bloom_upsample_add(upper, lower) if dual else orc.blur_h(lower, ow, oh), ow, oh)
    d = common.half_ulp_diff(got, staged)
    print(f"k_blur_up_poly {lw}x{lh} dual={dual}: interval at most {r['width']} wide, {r['degenerate']:.2%} degenerate; "
          f"{int((d > 0).sum())} of {d.size} values differ from the oracle's two calls (at most {int(d.max())} ULP), all inside the interval")


def test_shader_order_kernel_with_32_row_tiles(ctx, orc):
    """960 x 480 -> 1920 x 960 under set_bloom_shader_order: 900 tiles of 64 x 32, the TH = 32 instance of k_blur_hv"""
    lw, lh, ow, oh = 960, 480, 1920, 960
    lower, upper = bt.plane("noise", lw, lh, seed=9), bt.plane("noise", ow, oh, seed=10)
    ctx.set_bloom_shader_order(True)
    try:
        got = _up_level(ctx, lower, upper, ow, oh)
    finally:
        ctx.set_bloom_shader_order(False)
    lo, hi = bt.up_level_interval(upper, lower, ow, oh)
    r = bt.check_chain(got, lo, hi, "shader-order up_level 960x480")
    staged = orc.blur_v(orc.bloom_upsample_add(upper, lower), ow, oh)
    print(f"k_blur_hv TH=32 {lw}x{lh}: interval at most {r['width']} wide, {r['degenerate']:.2%} degenerate; "
          f"{int((got.view(np.uint16) != staged.view(np.uint16)).sum())} values differ from the oracle's two calls")
