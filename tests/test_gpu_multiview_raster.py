"""The sky resolve of N views per launch on the GPU (include/pbr_hip.h: pbr_skybox_views, pbr_skybox_bc6h_views;
pipeline.MultiViewFrame.skybox): every view's HDR target is bit-identical to its own single-view call's — which
tests/test_gpu_cameras.py and tests/test_gpu_sky_bc6h.py hold to their references — pixels under geometry and everything outside
w x h keep what they held, refused calls enqueue nothing, and a MultiViewFrame with a sky renders what one DeferredFrame per view
renders.  Reads tests/golden/ only."""
import os

import numpy as np
import pytest
import torch

import camera_cases
import common
from direct12pbrrenderer_amd import host, scene, synth
from direct12pbrrenderer_amd.api import PbrError
from direct12pbrrenderer_amd.pipeline import DeferredFrame, MultiViewFrame, ResidentSky, TileSpec
from direct12pbrrenderer_amd.structs import MAX_VIEWS, Tile, View

pytestmark = pytest.mark.gpu

GUARD = 3                    # sentinel rows above and below a target
HDR_SENTINEL = 0x7A5C        # the half every target pixel holds before a resolve


@pytest.fixture(scope="module")
def sky_file(ctx):
    """tests/golden/sky_bc6h.npz's smooth file on the device: its faces' addresses, size, mips, and the decoded fp32 cube"""
    data = np.load(os.path.join(common.ROOT, "tests", "golden", "sky_bc6h.npz"), allow_pickle=False)["smooth_file"]
    size, mips, offsets, _ = host.parse_cubemap_file(data.tobytes())
    staged = ctx.upload(data.copy())
    faces = [staged.data_ptr() + o for o in offsets]
    cube = ctx.bc6h_decode_cube(faces, size, mips)
    ctx.sync()
    return dict(staged=staged, faces=faces, size=size, mips=mips, cube=cube)


def sky_camera(k, w, h):
    """view k: camera_cases' cameras in turn, the ones that pitch and roll first, each round of them rolled, turned and pitched
    further (the sky sees the rotation only)"""
    name = camera_cases.NAMES[(k + 1) % len(camera_cases.NAMES)]
    cam = camera_cases.camera(name, w, h)
    step = k // len(camera_cases.NAMES)
    cam.rotate(0.23 * step, 0.71 * step, -0.17 * step)
    return cam


def hdr_target(ctx, h, pitch):
    return ctx.empty((h + 2 * GUARD, pitch, 4), torch.int16).fill_(HDR_SENTINEL)


def sky_views(globals_, stencils, pitch, targets, hdr_pitch):
    views = (View * len(globals_))()
    for k, g in enumerate(globals_):
        views[k].g = g
        views[k].gb.stencil = stencils[k].data_ptr()
        views[k].gb.pitch = pitch
        views[k].hdr = targets[k][GUARD:].data_ptr()
        views[k].hdr_pitch = hdr_pitch
    return views


@pytest.mark.parametrize("w,h,n", [(70, 45, 3), (256, 144, 16)])
def test_sky_views_bit_identical_to_single_view_calls(ctx, sky_file, w, h, n):
    """pbr_skybox_views and pbr_skybox_bc6h_views under stencil masks that cover part of each frame, planes with pitch > w and guard
    rows: every HDR target equals the per-view call's, covered pixels and everything outside w x h keep the sentinel"""
    rng = np.random.default_rng(w)
    globals_ = [scene.make_global(sky_camera(k, w, h), w, h) for k in range(n)]
    pitch, hdr_pitch = w + 3, w + 5
    masks = []
    for k in range(n):         # 8 x 8 blocks of geometry over about 40 % of the frame, another pattern per view
        m = (rng.random(((h + 7) // 8, (w + 7) // 8)) < 0.4).astype(np.uint8) * (1 + k)
        masks.append(np.repeat(np.repeat(m, 8, axis=0), 8, axis=1)[:h, :w])
    stencils = [ctx.upload(np.ascontiguousarray(np.pad(m, ((0, 0), (0, pitch - w)), constant_values=0))) for m in masks]
    tile = Tile(0, 0, w, h, w, h)
    s = sky_file
    for kind in ("f32", "bc6h"):
        want = [hdr_target(ctx, h, hdr_pitch) for _ in range(n)]
        got = [hdr_target(ctx, h, hdr_pitch) for _ in range(n)]
        for k in range(n):
            if kind == "f32":
                ctx.skybox(globals_[k], tile, s["cube"], s["size"], s["mips"], stencils[k], pitch, want[k][GUARD:], hdr_pitch)
            else:
                ctx.skybox_bc6h(globals_[k], tile, s["faces"], s["size"], s["mips"], stencils[k], pitch, want[k][GUARD:], hdr_pitch)
        views = sky_views(globals_, stencils, pitch, got, hdr_pitch)
        if kind == "f32":
            ctx.skybox_views(views, n, w, h, s["cube"], s["size"], s["mips"])
        else:
            ctx.skybox_bc6h_views(views, n, w, h, s["faces"], s["size"], s["mips"])
        ctx.sync()
        for k in range(n):
            a, b = got[k].cpu().numpy().view(np.uint16), want[k].cpu().numpy().view(np.uint16)
            assert np.array_equal(a, b), (kind, k, int((a != b).any(axis=-1).sum()))
            inner = a[GUARD:GUARD + h, :w]
            assert (inner[masks[k] != 0] == HDR_SENTINEL).all() and (inner[masks[k] == 0][:, 3] == 0x3C00).all(), (kind, k)
            assert (a[:GUARD] == HDR_SENTINEL).all() and (a[GUARD + h:] == HDR_SENTINEL).all() and (a[:, w:] == HDR_SENTINEL).all(), (kind, k)
            assert len(np.unique(inner[masks[k] == 0][:, :3], axis=0)) > 10, (kind, k)
        assert not np.array_equal(got[0].cpu().numpy(), got[1].cpu().numpy())


def test_refused_sky_calls_enqueue_nothing(ctx, sky_file):
    """n = 0, n = 17, a null target, view 1's target starting inside view 0's, pitches below w, a null cube: PBR_ERR_INVALID with a
    message, and the sentinel-filled targets stay sentinel"""
    w, h, n = 70, 45, 3
    s = sky_file
    globals_ = [scene.make_global(sky_camera(k, w, h), w, h) for k in range(MAX_VIEWS + 1)]
    stencils = [ctx.zeros((h, w), torch.uint8) for _ in globals_]
    targets = [hdr_target(ctx, h, w) for _ in globals_]

    def null_target(a):
        a[1].hdr = None

    def null_stencil(a):
        a[2].gb.stencil = None

    def overlap(a):           # view 1's target starts inside view 0's
        a[1].hdr = a[0].hdr + 8 * w * 10

    def narrow_pitch(a):
        a[0].gb.pitch = w - 1

    def narrow_hdr_pitch(a):
        a[2].hdr_pitch = w - 1
    cases = {"0 views": dict(n=0), "17 views": dict(n=MAX_VIEWS + 1), "a null target": dict(edit=null_target),
             "a null stencil plane": dict(edit=null_stencil), "overlapping targets": dict(edit=overlap), "pitch < w": dict(edit=narrow_pitch),
             "hdr pitch < w": dict(edit=narrow_hdr_pitch), "zero width": dict(w=0)}
    for what, kw in cases.items():
        views = sky_views(globals_, stencils, w, targets, w)
        if "edit" in kw:
            kw["edit"](views)
        for call in (lambda: ctx.skybox_views(views, kw.get("n", n), kw.get("w", w), h, s["cube"], s["size"], s["mips"]),
                     lambda: ctx.skybox_bc6h_views(views, kw.get("n", n), kw.get("w", w), h, s["faces"], s["size"], s["mips"])):
            with pytest.raises(PbrError, match="pbr_skybox") as e:
                call()
            assert "views" in str(e.value), what
    views = sky_views(globals_, stencils, w, targets, w)
    with pytest.raises(PbrError, match="pbr_skybox_views"):
        ctx.skybox_views(views, n, w, h, s["cube"], s["size"], s["mips"] + 1)
    with pytest.raises(PbrError, match="pbr_skybox_bc6h_views"):
        ctx.skybox_bc6h_views(views, n, w, h, s["faces"], 6, 1)
    ctx.sync()
    for t in targets:
        assert (t.cpu().numpy().view(np.uint16) == HDR_SENTINEL).all()
    ctx.skybox_views(views, n, w, h, s["cube"], s["size"], s["mips"])        # and the good call does run
    ctx.sync()
    assert not (targets[0][GUARD:GUARD + h].cpu().numpy().view(np.uint16) == HDR_SENTINEL).any()


def bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy() if t.dtype == torch.float16 else t.contiguous().view(torch.int32).cpu().numpy()


@pytest.mark.parametrize("w,h,n", [(256, 144, 3), (64, 48, MAX_VIEWS + 2)])
def test_frames_with_a_sky_match_deferred_frames(ctx, ibl, sky_file, w, h, n):
    """MultiViewFrame.render() with an fp32 sky and with a ResidentSky (one sky call per batch of MAX_VIEWS: 18 views take two)
    against one DeferredFrame per view with the same inputs: HDR target, LDR output and adapted luminance"""
    _, env, lut, sh = ibl

    def dev_half(a):
        return ctx.upload(np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)).view(torch.float16)
    lut_d, env_d = dev_half(lut), dev_half(env)
    cams = [sky_camera(k, w, h) for k in range(n)]
    globals_ = [scene.make_global(c, w, h, sh_pack=sh, delta_time=1.0 / 60.0 + 0.001 * k) for k, c in enumerate(cams)]
    lights = [camera_cases.lights_around((8, 0, 40)[k % 3], c) for k, c in enumerate(cams)]
    gbs = [synth.gbuffer_tile(0, 0, w, h, w, h, near=float(c.near), far=float(c.far), coverage_mask=True, cell=1 + k % 3)
           for k, c in enumerate(cams)]
    assert all((gb["stencil"] == 0).sum() > 0.05 * w * h for gb in gbs)
    s = sky_file
    lum = [0.1 + 0.02 * k for k in range(n)]
    for kind, sky in (("f32", (s["cube"], s["size"], s["mips"])), ("resident", ResidentSky(s["staged"], s["faces"], s["size"], s["mips"]))):
        mv = MultiViewFrame(ctx, w, h, globals_, lights, lut_d, lut.shape[0], env_d, common.ENV_SIZE, common.ENV_MIPS, sky=sky)
        mv.upload_gbuffers(gbs)
        mv.set_prev_luminance(lum)
        mv.render()
        ctx.sync()
        for k in range(n):
            fr = DeferredFrame(ctx, TileSpec(0, 0, w, h, w, h, 0), globals_[k], lights[k], lut_d, lut.shape[0], env_d, common.ENV_SIZE,
                               common.ENV_MIPS, sky=sky)
            fr.upload_gbuffer(gbs[k])
            fr.set_prev_luminance(lum[k])
            fr.render()
            ctx.sync()
            assert np.array_equal(bits(mv.hdr(k)), bits(fr.hdr)), (kind, k, "HDR")
            assert np.array_equal(mv.ldr_numpy(k), fr.ldr_numpy()), (kind, k, "LDR")
            assert np.array_equal(bits(mv.avg[k]), bits(fr.avg)), (kind, k, "adapted luminance")
        assert not np.array_equal(bits(mv.hdr(0)), bits(mv.hdr(1)))
