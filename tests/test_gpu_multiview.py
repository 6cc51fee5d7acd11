"""Multi-view frames (pbr_*_views, pipeline.MultiViewFrame): every view of a batch is bit-identical to the same inputs through
their own DeferredFrame — HDR, histogram, adapted luminance, LDR — and the entry points refuse bad batches without touching
their outputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import common
from direct12pbrrenderer_amd import scene, synth
from direct12pbrrenderer_amd.api import PbrContext, PbrError
from direct12pbrrenderer_amd.pipeline import DeferredFrame, MultiViewFrame, TileSpec
from direct12pbrrenderer_amd.structs import MAX_VIEWS, View

pytestmark = pytest.mark.gpu

LIGHT_COUNTS = (0, 8, 256, 1024)   # both LDS strides (<= 256 and 1025)


@pytest.fixture(scope="module")
def ctx():
    c = PbrContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ibl(ctx):
    from oracle import binding as orc
    sky, env, lut, sh = common.small_ibl(orc)

    def dev_half(a):
        return ctx.upload(np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)).view(torch.float16)
    return dict(orc=orc, sky=sky, env_np=env, lut_np=lut, sh=sh, env=dev_half(env), lut=dev_half(lut))


def view_inputs(v, W, H, sh, n_lights, delta_time=1.0 / 60.0):
    """view v: its own camera (yaw, Fov, Near / Far), G-buffer and lights"""
    fov = np.float32(0.333 + 0.04 * (v % 3)) * np.float32(np.pi)
    near, far = (0.1, 1000.0) if v % 2 == 0 else (0.25, 400.0)
    cam = scene.Camera(fov, W, H, near, far)
    cam.move((0.3 * v, 3.0, 10.0 - 0.5 * v))
    cam.rotate(0.0, float(np.pi) + 0.15 * v, 0.0)
    g = scene.make_global(cam, W, H, sh_pack=sh, delta_time=delta_time)
    if n_lights == 0:
        lights = scene.make_lights(np.zeros((0, 3)), np.zeros((0, 3)), 2.0, 10.0)
    else:
        lights = synth.lights_in_view_box(n_lights, cam, seed=0x5EED0100 + v)
    gb = synth.gbuffer_tile(0, 0, W, H, W, H, near=near, far=far, rough_min=48, coverage_mask=True, cell=1 + v % 3)
    return g, lights, gb


def make_pair(ctx, ibl, W, H, n_views, lum=None, dts=None):
    """a MultiViewFrame of n_views views and one DeferredFrame per view on the same inputs"""
    ins = [view_inputs(v, W, H, ibl["sh"], LIGHT_COUNTS[v % len(LIGHT_COUNTS)], dts[v] if dts else 1.0 / 60.0) for v in range(n_views)]
    mv = MultiViewFrame(ctx, W, H, [i[0] for i in ins], [i[1] for i in ins], ibl["lut"], ibl["lut_np"].shape[0], ibl["env"],
                        common.ENV_SIZE, common.ENV_MIPS)
    mv.upload_gbuffers([i[2] for i in ins])
    lum = lum or [0.18 + 0.05 * v for v in range(n_views)]
    mv.set_prev_luminance(lum)
    singles = []
    for v, (g, lights, gb) in enumerate(ins):
        fr = DeferredFrame(ctx, TileSpec(0, 0, W, H, W, H, 0), g, lights, ibl["lut"], ibl["lut_np"].shape[0], ibl["env"],
                           common.ENV_SIZE, common.ENV_MIPS)
        fr.upload_gbuffer(gb)
        fr.set_prev_luminance(lum[v])
        singles.append(fr)
    return mv, singles


def bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy() if t.dtype == torch.float16 else t.contiguous().view(torch.int32).cpu().numpy()


# 1279x719: level 0 is not an exact half, so the prefilter and the level-0 tail take the staged kernels, once per view
@pytest.mark.parametrize("W,H,n_views", [(1440, 960, 4), (1920, 1080, 3), (3840, 2160, 2), (256, 144, 5), (1279, 719, 2)])
def test_views_bit_identical_to_single_views(ctx, ibl, W, H, n_views):
    mv, singles = make_pair(ctx, ibl, W, H, n_views)
    # stage by stage: the histogram is cleared by the average, so it is compared before it
    mv.clustered()
    mv.shade()
    mv.bloom_histogram()
    for fr in singles:
        fr.clustered()
        fr.shade()
        fr.bloom_histogram()
    ctx.sync()
    for v, fr in enumerate(singles):
        assert np.array_equal(bits(mv.clusters[v]), bits(fr.clusters)), f"view {v}: cluster lists differ"
        assert np.array_equal(bits(mv.hdr(v)), bits(fr.hdr)), f"view {v} ({W}x{H}, {fr.n_lights} lights): HDR differs"
        assert np.array_equal(bits(mv.hist[v]), bits(fr.hist)), f"view {v}: histogram differs"
        assert int(fr.hist.sum()) == W * H
    mv.average()
    mv.tonemap()
    for fr in singles:
        fr.average()
        fr.tonemap()
    ctx.sync()
    for v, fr in enumerate(singles):
        assert np.array_equal(bits(mv.avg[v]), bits(fr.avg)), f"view {v}: adapted luminance differs"
        assert np.array_equal(mv.ldr_numpy(v), fr.ldr_numpy()), f"view {v}: LDR differs"
        assert not np.array_equal(bits(mv.hdr(v)), bits(mv.hdr((v + 1) % n_views))), "views must differ from each other"


def test_views_render_matches_deferred_frame_render(ctx, ibl):
    """MultiViewFrame.render() against DeferredFrame.render(), more views than one call takes (two calls)"""
    W, H, n = 256, 144, MAX_VIEWS + 2
    mv, singles = make_pair(ctx, ibl, W, H, n)
    mv.render()
    for fr in singles:
        fr.render()
    ctx.sync()
    for v, fr in enumerate(singles):
        assert np.array_equal(bits(mv.hdr(v)), bits(fr.hdr)), f"view {v}: HDR differs"
        assert np.array_equal(bits(mv.avg[v]), bits(fr.avg)), f"view {v}: adapted luminance differs"
        assert np.array_equal(mv.ldr_numpy(v), fr.ldr_numpy()), f"view {v}: LDR differs"


def test_views_temporal_exposure(ctx, ibl):
    """five frames, per-view DeltaTime and starting luminance: every view's adapted luminance follows its own DeferredFrame"""
    W, H, n = 256, 144, 3
    dts = [1.0 / 60.0, 1.0 / 30.0, 0.25]
    mv, singles = make_pair(ctx, ibl, W, H, n, lum=[0.05, 0.18, 2.0], dts=dts)
    seen = []
    for frame in range(5):
        mv.render()
        for fr in singles:
            fr.render()
        ctx.sync()
        got = [float(a.cpu()[0]) for a in mv.avg]
        for v, fr in enumerate(singles):
            assert np.array_equal(bits(mv.avg[v]), bits(fr.avg)), f"frame {frame}, view {v}: {got[v]} vs {float(fr.avg.cpu()[0])}"
        seen.append(got)
    assert len({tuple(s) for s in seen}) == 5, "the luminance must move from frame to frame"


def test_views_against_oracle(ctx, ibl):
    """one view of a 4-view 256x144 batch, checked like smoke(): bloom -> histogram -> average -> tone-map against the oracle on the
    oracle's own shade, and the shade itself (fp32 probe of the same view) against the f64 evaluation"""
    orc = ibl["orc"]
    W, H = 256, 144
    ins = [view_inputs(v, W, H, ibl["sh"], (8, 256, 0, 1024)[v]) for v in range(4)]
    _, g, lights, gb, tile = common.shade_scene(W, H, 256, ibl["sh"], rough_min=48, coverage_mask=True)
    k = 1
    ins[k] = (g, lights, gb)
    mv = MultiViewFrame(ctx, W, H, [i[0] for i in ins], [i[1] for i in ins], ibl["lut"], ibl["lut_np"].shape[0], ibl["env"],
                        common.ENV_SIZE, common.ENV_MIPS)
    mv.upload_gbuffers([i[2] for i in ins])
    mv.set_prev_luminance(0.18)
    mv.render()
    ctx.sync()
    got_hdr = mv.hdr(k).cpu().view(torch.int16).numpy().view(np.float16)
    got_ldr = mv.ldr_numpy(k)
    lut, env = ibl["lut_np"], ibl["env_np"]
    cl = orc.cluster_build(g)
    orc.cluster_cull(g, lights, cl)
    hdr, hdr32 = orc.deferred_shade(g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights, want_f32=True)
    lo, hi, flags = orc.deferred_shade_f64(g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights)
    out32 = ctx.zeros((H, W, 4), torch.float32)
    gbd = mv.gb[k]
    ctx.deferred_shade_f32(g, mv.tile, gbd, W, mv.lut, mv.lut_res, mv.env, mv.env_size, mv.env_mips, mv.clusters[k], mv.lights[k],
                           mv.n_lights[k], out32, W)
    ctx.sync()
    ok = flags == 0
    assert ok.mean() > 0.85
    s32 = float(np.abs(hi[ok]).max())
    d_gpu, d_orc = orc.truth_distance(out32.cpu().numpy(), lo, hi)[ok], orc.truth_distance(hdr32, lo, hi)[ok]
    assert float((d_gpu / (1e-4 * s32 + 4.0 * d_orc)).max()) <= 1.0
    orc.bloom(hdr)
    hist = orc.lum_histogram(hdr)
    avg = orc.lum_average(hist, W * H, float(g.DeltaTime), 0.18)
    ldr = orc.tonemap(hdr, avg)
    on = gb["stencil"] > 0
    scale = float(np.abs(hdr.astype(np.float32)[on][:, :3]).max())
    err = float(np.abs(got_hdr.astype(np.float32) - hdr.astype(np.float32))[on][:, :3].max())
    assert err <= (1e-4 + 2.0 ** -10) * scale, f"HDR L-inf {err} (scale {scale})"
    dl = np.abs(((got_ldr[..., None] >> np.array([0, 8, 16], dtype=np.uint32)) & 255).astype(np.int32)
                - ((ldr[..., None] >> np.array([0, 8, 16], dtype=np.uint32)) & 255).astype(np.int32))
    assert (dl > 1).mean() < 1e-3
    assert abs(float(mv.avg[k].cpu()[0]) - avg) <= 1e-4 * abs(avg) + 1e-7


# ---- validation: PBR_ERR_INVALID with a message, nothing enqueued, outputs untouched
def test_views_validation(ctx, ibl):
    W, H, n = 256, 144, 3
    mv, _ = make_pair(ctx, ibl, W, H, n)
    lib, h = ctx.lib, ctx.h
    for v in range(n):
        mv.hdrs[v].view(torch.int16).fill_(0x1234)
        mv.ldr[v].fill_(0x5A5A5A5A)
        mv.hist[v].fill_(7)
        mv.avg[v].fill_(3.0)
        mv.clusters[v].fill_(0x3C)
    ctx.sync()
    before = [(bits(mv.hdrs[v]).copy(), mv.ldr_numpy(v).copy(), bits(mv.hist[v]).copy(), bits(mv.avg[v]).copy(), bits(mv.clusters[v]).copy())
              for v in range(n)]
    lut, env, lr = mv.lut, mv.env, mv.lut_res

    def calls(arr, k):
        return {
            "clustered": lambda: lib.pbr_clustered_views(h, arr, k),
            "shade": lambda: lib.pbr_deferred_shade_views(h, arr, k, W, H, C.c_void_p(lut.data_ptr()), lr, C.c_void_p(env.data_ptr()),
                                                          common.ENV_SIZE, common.ENV_MIPS),
            "bloom": lambda: lib.pbr_bloom_histogram_views(h, arr, k, W, H, 1.0, 0.5, -10.0, 1.0 / 12.0),
            "average": lambda: lib.pbr_lum_average_views(h, arr, k, W * H, -10.0, 12.0),
            "tonemap": lambda: lib.pbr_tonemap_views(h, arr, k, W, H),
        }

    def views(edit=None):
        arr = (View * (MAX_VIEWS + 1))(*[mv._view(v % n) for v in range(MAX_VIEWS + 1)])
        if edit:
            edit(arr)
        return arr

    def expect_invalid(name, fn, what):
        st = fn()
        msg = (lib.pbr_last_error(h) or b"").decode()
        assert st == -1, f"{name}: {what} accepted (status {st})"
        assert msg.startswith("pbr_") and "views" in msg, f"{name}: {what}: message {msg!r}"

    base = views()
    for name, fn in calls(base, 0).items():
        expect_invalid(name, fn, "0 views")
    for name, fn in calls(base, MAX_VIEWS + 1).items():   # (views repeat: the count is checked first)
        expect_invalid(name, fn, f"{MAX_VIEWS + 1} views")
    for name, fn in calls(None, 2).items():
        expect_invalid(name, fn, "null view array")

    def null_plane(a):
        a[1].gb.B = None
    expect_invalid("shade", calls(views(null_plane), n)["shade"], "null G-buffer plane")

    def null_hist(a):
        a[2].hist256 = None
    for name in ("bloom", "average"):
        expect_invalid(name, calls(views(null_hist), n)[name], "null histogram")

    def other_sh(a):
        a[1].g.SkyBoxSH.sha_r[0] += 1.0
    expect_invalid("shade", calls(views(other_sh), n)["shade"], "SkyBoxSH differing between views")

    def too_many_lights(a):
        a[0].num_lights = 1025
    for name in ("clustered", "shade"):
        expect_invalid(name, calls(views(too_many_lights), n)[name], "1025 lights")

    def bad_near(a):
        a[2].g.Near = 0.0
    for name in ("clustered", "shade"):
        expect_invalid(name, calls(views(bad_near), n)[name], "Near = 0")

    def narrow_pitch(a):
        a[0].hdr_pitch = W - 2
    for name in ("shade", "bloom", "tonemap"):
        expect_invalid(name, calls(views(narrow_pitch), n)[name], "pitch < width")

    shared = {"clustered": ("clusters",), "shade": ("hdr",), "bloom": ("hdr", "chain_a", "chain_b", "hist256"),
              "average": ("hist256", "avg"), "tonemap": ("rgba8",)}
    for name, fields in shared.items():
        for f in fields:
            def share(a, f=f):
                setattr(a[2], f, getattr(a[0], f))
            expect_invalid(name, calls(views(share), n)[name], f"two views sharing {f}")

    def overlap(a):   # view 1's HDR target starts inside view 0's
        a[1].hdr = a[0].hdr + 8 * W * 10
    expect_invalid("shade", calls(views(overlap), n)["shade"], "overlapping HDR targets")

    def cross(a):     # view 1's chain A is view 0's HDR target
        a[1].chain_a = a[0].hdr
    expect_invalid("bloom", calls(views(cross), n)["bloom"], "a chain on another view's HDR target")
    expect_invalid("tonemap", lambda: lib.pbr_tonemap_views(h, base, n, 0, H), "zero width")
    assert lib.pbr_clustered_views(None, base, n) == -1

    ctx.sync()
    for v in range(n):
        after = (bits(mv.hdrs[v]), mv.ldr_numpy(v), bits(mv.hist[v]), bits(mv.avg[v]), bits(mv.clusters[v]))
        for b, a, what in zip(before[v], after, ("HDR", "LDR", "histogram", "avg", "clusters")):
            assert np.array_equal(b, a), f"view {v}: {what} changed by a refused call"
    # the same buffers are accepted as they are
    mv.render()
    ctx.sync()
    with pytest.raises(PbrError):
        ctx.tonemap_views(base, 0, W, H)
