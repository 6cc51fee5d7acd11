"""DeferredFrame.set_sun on the GPU: a ground quad and a box at 256 x 144.  The HDR target before the bloom equals the frame without
a sun plus the pbr_sun_light call made by hand, bit for bit; set_sun(None) restores the frame; the shadow map is rasterized once per
set_meshes / set_sun; inside the box's analytic shadow the added light is 0 and on the open ground it is the unshadowed closed form
(tests/sun_truth.py) within the probe's bound.  HostRenderer.set_sun_light: the C++ pass graph's frame equals the Python-driven one bit for
bit, dispatch by dispatch and fused, and with the sun off its order list, dispatch count and frame are the parent's."""
import math

import numpy as np
import pytest
import torch

import common
import sun_truth as st
from direct12pbrrenderer_amd import api, scene
from direct12pbrrenderer_amd.pipeline import DeferredFrame, TileSpec
from direct12pbrrenderer_amd.structs import Tile

W, H, MAP = 256, 144, 256
GROUND_Y = -1.5
BOX = ((-2.0, GROUND_Y, 5.0), (0.5, 0.5, 7.5))          # view space, standing on the ground, two units tall
SUN_VIEW = np.array([math.sin(0.6) * math.cos(2.4), math.cos(0.6), math.sin(0.6) * math.sin(2.4)])      # 34 degrees off the view's up axis
BIAS = (4e-3, 3.2e-2)    # a 256^2 map has 8 x the texel of the default 2048^2 one: DeferredFrame.SUN_BIAS scaled by 8
MAP2, BIAS2 = 96, (1.1e-2, 8.5e-2)      # a second map size for the host graph's resize sequence, its bias scaled alike


def face_model(inv_view, centre, normal, x_axis):
    """quad_grid's plane (facing -z) placed at `centre` of view space with its front towards `normal`: a proper rotation"""
    z = -np.asarray(normal, dtype=np.float64)
    x = np.asarray(x_axis, dtype=np.float64)
    y = np.cross(z, x)
    to_view = np.eye(4)
    to_view[:3, 0], to_view[:3, 1], to_view[:3, 2], to_view[:3, 3] = x, y, z, centre
    assert abs(np.linalg.det(to_view[:3, :3]) - 1.0) < 1e-12
    return (inv_view @ to_view).astype(np.float32)


def box_scene(g):
    inv_view = np.array(g.InvView[:], dtype=np.float64).reshape(4, 4)
    ms = scene.MeshScene()
    ms.add(scene.quad_grid(4, 4, size=(10.0, 9.0)), face_model(inv_view, (0.0, GROUND_Y, 7.0), (0, 1, 0), (1, 0, 0)), albedo=(0.8, 0.7, 0.6),
           roughness=0.6, metallic=0.1)
    (x0, y0, z0), (x1, y1, z1) = BOX
    cx, cy, cz = 0.5 * (x0 + x1), 0.5 * (y0 + y1), 0.5 * (z0 + z1)
    faces = [((cx, y1, cz), (0, 1, 0), (1, 0, 0), (x1 - x0, z1 - z0)), ((x0, cy, cz), (-1, 0, 0), (0, 0, 1), (z1 - z0, y1 - y0)),
             ((x1, cy, cz), (1, 0, 0), (0, 0, 1), (z1 - z0, y1 - y0)), ((cx, cy, z0), (0, 0, -1), (1, 0, 0), (x1 - x0, y1 - y0)),
             ((cx, cy, z1), (0, 0, 1), (1, 0, 0), (x1 - x0, y1 - y0))]
    for centre, normal, x_axis, size in faces:
        ms.add(scene.quad_grid(1, 1, size=size), face_model(inv_view, centre, normal, x_axis), albedo=(0.3, 0.5, 0.9), roughness=0.4, metallic=0.5)
    return ms


@pytest.fixture(scope="module")
def frame(ctx, orc, ibl):
    sky, env, lut, sh = ibl
    cam = scene.Camera.reference_default(W, H)
    g = scene.make_global(cam, W, H, sh_pack=sh)

    def dev_half(a):
        return ctx.upload(np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)).view(torch.float16)
    from direct12pbrrenderer_amd import synth
    fr = DeferredFrame(ctx, TileSpec(0, 0, W, H, W, H, 0), g, synth.reference_scene_light(), dev_half(lut), lut.shape[0], dev_half(env),
                       common.ENV_SIZE, common.ENV_MIPS, sky=(ctx.upload(sky), common.SKY_SIZE, common.SKY_MIPS))
    # (with a sky every pixel of the HDR target is rewritten by every frame: without one the sky pixels keep the last frame's bloom)
    ms = box_scene(g)
    fr.set_meshes(*ms.arrays())
    fr.set_prev_luminance(0.18)
    inv_view = np.array(g.InvView[:], dtype=np.float64).reshape(4, 4)[:3, :3]
    return fr, g, ms, inv_view @ SUN_VIEW


def render_capturing_hdr(fr, **kw):
    """render() from the same adapted luminance every time (the exposure carries it from frame to frame); returns (the HDR target as the
    bloom found it, the LDR image)"""
    fr.set_prev_luminance(0.18)
    seen = {}
    bloom = fr.bloom_histogram

    def spy():
        seen["hdr"] = fr.hdr.clone()
        bloom()
    fr.bloom_histogram = spy
    try:
        fr.render(**kw)
    finally:
        del fr.bloom_histogram
    fr.ctx.sync()
    return seen["hdr"].cpu().view(torch.int16).numpy(), fr.ldr_numpy().copy()


def count_rasters(fr):
    calls = []
    real = fr.ctx.gbuffer_raster

    def spy(g, tile, *a, **k):
        calls.append((tile.w, tile.h))
        return real(g, tile, *a, **k)
    fr.ctx.gbuffer_raster = spy
    return calls


@pytest.mark.gpu
def test_frame_with_sun_is_the_frame_plus_the_call_by_hand(ctx, orc, frame):
    fr, g, ms, sun_dir = frame
    fr.set_sun(None)
    hdr0, ldr0 = render_capturing_hdr(fr)
    calls = count_rasters(fr)
    try:
        fr.set_sun(sun_dir, (100.0, 90.0, 70.0), map_size=MAP, pcf=3, bias=BIAS)
        hdr1, ldr1 = render_capturing_hdr(fr)
        hdr1b, _ = render_capturing_hdr(fr)
        assert calls.count((MAP, MAP)) == 1 and calls.count((W, H)) == 2, calls      # the shadow map once, the camera's G-buffer per frame
        fr.refresh_shadow_map()
        render_capturing_hdr(fr)
        assert calls.count((MAP, MAP)) == 2
    finally:
        del fr.ctx.gbuffer_raster
    assert np.array_equal(hdr1, hdr1b) and not np.array_equal(hdr1, hdr0) and not np.array_equal(ldr1, ldr0)
    # by hand: fit, rasterize the map, one pbr_sun_light on the no-sun HDR
    v, i, d = ms.arrays()
    mn, mx = scene.world_box(d, ms.bounds())
    light_g, lvp = api.sun_fit((sun_dir / np.linalg.norm(sun_dir)).astype(np.float32), mn, mx, MAP, MAP)
    n = int((d["index_count"] // 3).sum())
    planes = [ctx.zeros((MAP, MAP), torch.int32) for _ in range(3)]
    depth, stencil = ctx.zeros((MAP, MAP), torch.float32), ctx.zeros((MAP, MAP), torch.uint8)
    ctx.gbuffer_raster(light_g, Tile(0, 0, MAP, MAP, MAP, MAP), ctx.upload(v), len(v), ctx.upload(i), len(i), ctx.upload(d), len(d), n, *planes,
                       depth, stencil, MAP, ctx.alloc_raster_scratch(MAP, MAP, n))
    sun = api.make_sun(sun_dir, (100.0, 90.0, 70.0), lvp, BIAS, 3)
    hdr = ctx.upload(hdr0).view(torch.float16)
    ctx.sun_light(g, fr.tile, fr.gb, W, sun, hdr, W, depth, MAP, MAP, MAP)
    ctx.sync()
    assert np.array_equal(hdr.cpu().view(torch.int16).numpy(), hdr1)
    # set_sun(None): today's frame, bit for bit
    fr.set_sun(None)
    hdr2, ldr2 = render_capturing_hdr(fr)
    assert np.array_equal(hdr2, hdr0) and np.array_equal(ldr2, ldr0)

    # the added light against the analytic shadow of the box and the closed form on the open ground
    probe = ctx.zeros((H, W, 4), torch.float32)
    ctx.sun_light(g, fr.tile, fr.gb, W, sun, None, W, depth, MAP, MAP, MAP, contrib_f32=probe)
    ctx.sync()
    probe = probe.cpu().numpy()
    gb = {k: t.cpu().numpy() for k, t in fr.gb.items()}
    gb = {k: (p.view(np.uint32) if k in "ABC" else p) for k, p in gb.items()}
    tile = Tile(0, 0, W, H, W, H)
    s = st.make_sun(sun_dir, (100.0, 90.0, 70.0))
    tr = st.truth(st.camera_of(g), tile, gb, s)                 # vis = 1: the unshadowed closed form
    restated = st.restate(st.camera_of(g), tile, gb, s)
    view = np.array(g.View[:], dtype=np.float64).reshape(4, 4)
    pv = tr["position"] @ view[:3, :3].T + view[:3, 3]
    ground = tr["on"] & (np.abs(pv[..., 1] - GROUND_Y) < 0.02)
    # a ground point is in shadow iff the ray towards the sun meets the box: slabs.  `grow` widens (> 0) or shrinks (< 0) the box by the
    # tolerance: 2.5 map texels of the pcf-3 footprint (stretched where the tilted light meets the ground) plus the pixel's own size
    texel = 2.5 * math.hypot(*[(mx[k] - mn[k]) for k in (0, 2)]) / (MAP - 2) / SUN_VIEW[1]
    step = np.maximum(np.linalg.norm(np.gradient(pv, axis=1), axis=-1), np.linalg.norm(np.gradient(pv, axis=0), axis=-1))

    def hits(grow):
        lo = np.array(BOX[0])[None, None, :] - grow[..., None]
        hi = np.array(BOX[1])[None, None, :] + grow[..., None]
        lo[..., 1] = BOX[0][1] - 1.0        # the box stands on the ground: its base is not an edge of the shadow
        with np.errstate(all="ignore"):
            t0, t1 = (lo - pv) / SUN_VIEW, (hi - pv) / SUN_VIEW
        near, far = np.minimum(t0, t1).max(axis=-1), np.maximum(t0, t1).min(axis=-1)
        return (near <= far) & (far > 0)
    tol = texel + step
    deep, open_ = ground & hits(-tol) & (tol < 0.45), ground & ~hits(tol)
    assert deep.sum() > 300 and open_.sum() > 5000, (int(deep.sum()), int(open_.sum()))
    assert not probe[deep][:, :3].any(), "light inside the box's analytic shadow"
    scale = tr["unshadowed"][open_].max(axis=-1, keepdims=True)
    err = np.abs(probe[open_][:, :3] - tr["contrib"][open_])
    bound = st.F32_REL * scale + st.RESTATEMENT_FACTOR * np.abs(restated[open_][:, :3] - tr["contrib"][open_])
    assert (err <= bound).all(), f"open ground: a pixel is {(err / bound).max():.3g} x its bound from the unshadowed closed form"


@pytest.mark.gpu
def test_set_sun_refusals_and_unshadowed_sun(ctx, orc, frame):
    fr, g, ms, sun_dir = frame
    fr.set_sun(sun_dir, 100.0, shadows=False)
    hdr_a, _ = render_capturing_hdr(fr)
    fr.set_sun(None)
    hdr0, _ = render_capturing_hdr(fr)
    hdr = ctx.upload(hdr0).view(torch.float16)
    ctx.sun_light(g, fr.tile, fr.gb, W, api.make_sun(sun_dir, 100.0, None, DeferredFrame.SUN_BIAS, 3), hdr, W)
    ctx.sync()
    assert np.array_equal(hdr.cpu().view(torch.int16).numpy(), hdr_a)
    with pytest.raises(ValueError):
        fr.set_sun(sun_dir, 100.0, depth_map=(hdr, 4, 4, 4))         # a map without its matrix
    gb_np = {k: t.cpu().numpy() for k, t in fr.gb.items()}
    try:
        fr.upload_gbuffer(gb_np)                                      # planes handed in directly: no meshes to cast shadows
        with pytest.raises(ValueError):
            fr.set_sun(sun_dir, 100.0)
        fr.set_sun(sun_dir, 100.0, shadows=False)
        fr.set_sun(None)
    finally:
        fr.set_meshes(*ms.arrays())


# ---- the C++ host graph: HostRenderer.set_sun_light
PARENT_ORDER = "PreFilterEnvMap>PrecomputeBRDF>Clustered>GBuffer>Skybox>DeferredShading>Bloom>AutoExposure>ToneMapping>Present"


def execution_order(r):
    import ctypes as C
    buf = C.create_string_buffer(512)
    assert r.lib.pbrh_execution_order(r.h, buf, 512) == 0
    return buf.value.decode()


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["dispatches", "fused"])
def test_host_renderer_sun_equals_the_python_frame(ctx, fused):
    """HostRenderer.set_sun_light: SunShadow after GBuffer, SunLight between DeferredShading and Bloom; the HDR target and the presented
    frame equal DeferredFrame.set_sun's bit for bit, dispatch by dispatch and fused; the map is rasterized once; with the sun off — before
    it was ever set and after it is cleared — the order list is the parent's, literally, and so are the dispatch count and the frame."""
    import ctypes as C
    from direct12pbrrenderer_amd import synth
    from direct12pbrrenderer_amd.host import HostError, HostRenderer
    from direct12pbrrenderer_amd.structs import LIGHT_DTYPE, Global
    ENV, LUT = 32, 64
    g_ref = scene.make_global(scene.Camera.reference_default(W, H), W, H)
    ms = box_scene(g_ref)
    v, i, d = ms.arrays()
    sun_dir = np.array(g_ref.InvView[:], dtype=np.float64).reshape(4, 4)[:3, :3] @ SUN_VIEW
    lights = synth.reference_scene_light()
    lum = (100.0, 90.0, 70.0)
    sky_np = synth.env_cube(ENV)
    r = HostRenderer(0, W, H, ENV, LUT)
    try:
        r.set_fused(fused)
        r.set_skybox(sky_np, ENV)
        r.set_lights(lights)
        r.set_meshes(v, i, d)

        def frame():
            r.set_initial_luminance(0.18)
            r.render(1.0 / 60.0)
            return (r.read("DeferredShadingRT", (H, W, 4), np.float16).view(np.uint16), r.read("ToneMappedTexture", (H, W), np.uint32),
                    r.dispatch_count())
        assert execution_order(r) == PARENT_ORDER
        frame()                                   # the one-shot IBL passes run in the first frame
        hdr_off, ldr_off, n_off = frame()
        r.set_sun_light(sun_dir, lum, map_size=MAP, pcf=3, bias=BIAS)
        order = execution_order(r).split(">")
        assert sorted(order) == sorted(PARENT_ORDER.split(">") + ["SunShadow", "SunLight"])
        pos = {n: k for k, n in enumerate(order)}
        assert pos["GBuffer"] < pos["SunShadow"] < pos["SunLight"] and pos["DeferredShading"] < pos["SunLight"] < pos["Bloom"]
        assert pos["Skybox"] < pos["SunLight"] and [n for n in order if not n.startswith("Sun")] == PARENT_ORDER.split(">")
        hdr_a, ldr_a, n_a = frame()
        hdr_b, ldr_b, n_b = frame()
        assert (n_a, n_b) == (n_off + 2, n_off + 1), (n_off, n_a, n_b)      # the shadow raster once, the light pass every frame
        assert np.array_equal(hdr_a, hdr_b) and np.array_equal(ldr_a, ldr_b) and not np.array_equal(hdr_a, hdr_off)
        shadow = r.read("SunShadowDepth", (MAP, MAP), np.float32)
        assert (shadow < 1.0).mean() > 0.1 and (shadow == 1.0).any()
        # a refused call after a valid one changes nothing: the earlier sun, its passes and its map stay
        for bad in (dict(direction=(0.0, 0.0, 0.0)), dict(direction=sun_dir, pcf=2), dict(direction=sun_dir, map_size=2),
                    dict(direction=(float("nan"), 1.0, 0.0))):
            with pytest.raises(HostError):
                r.set_sun_light(bad.pop("direction"), lum, **bad)
            assert execution_order(r).split(">") == order
        hdr_r, ldr_r, n_r = frame()
        assert n_r == n_off + 1 and np.array_equal(hdr_r, hdr_a) and np.array_equal(ldr_r, ldr_a)
        # an unshadowed sun: SunLight alone
        r.set_sun_light(sun_dir, lum, shadows=False)
        assert "SunShadow" not in execution_order(r) and "SunLight" in execution_order(r)
        hdr_u, _, n_u = frame()
        assert n_u == n_off + 1 and not np.array_equal(hdr_u, hdr_a)
        # off again: the parent's list, count and frame
        r.set_sun_light(None)
        assert execution_order(r) == PARENT_ORDER
        hdr_c, ldr_c, n_c = frame()
        assert n_c == n_off and np.array_equal(hdr_c, hdr_off) and np.array_equal(ldr_c, ldr_off)
        with pytest.raises(HostError):
            r.read("SunShadowDepth", (MAP, MAP), np.float32)       # the map went with the sun
        # a sun of another map size after the clear (and after an unshadowed one): the texture has the size asked for now
        r.set_sun_light(sun_dir, lum, map_size=MAP2, pcf=3, bias=BIAS2)
        hdr_s, ldr_s, n_s = frame()
        assert n_s == n_off + 2
        shadow2 = r.read("SunShadowDepth", (MAP2, MAP2), np.float32)
        with pytest.raises(HostError):
            r.read("SunShadowDepth", (MAP, MAP), np.float32)
        r.set_sun_light(sun_dir, lum, map_size=MAP, pcf=3, bias=BIAS)      # and resized while a sun is set
        hdr_t, ldr_t, _ = frame()
        assert np.array_equal(hdr_t, hdr_a) and np.array_equal(ldr_t, ldr_a)
        assert np.array_equal(r.read("SunShadowDepth", (MAP, MAP), np.float32), shadow)
        # what the Python-driven frame needs: the host's constant buffer and its light buffer
        g_host = Global()
        assert r.lib.pbrh_get_global(r.h, C.byref(g_host)) == 0
        packed = np.ascontiguousarray(np.concatenate([lights["Position"], lights["Color"], lights["Radius"][:, None], lights["Intensity"][:, None]],
                                                     axis=1), dtype=np.float32)
        buf = np.zeros(1024, LIGHT_DTYPE)
        cam4 = np.float32([0.0, 3.0, 10.0, 3.14159265359])
        n = r.lib.pbrh_light_buffer(W, H, cam4.ctypes.data, packed.ctypes.data, len(packed), buf.ctypes.data, 1024)
        assert n > 0
    finally:
        r.close()
    sky_mips = int(np.log2(ENV)) + 1
    sky = ctx.upload(sky_np)
    ctx.cube_gen_mips(sky, ENV, sky_mips)
    lut = ctx.brdf_lut(LUT)
    env = (ctx.prefilter_env if fused else ctx.prefilter_env_dispatches)(sky, ENV, sky_mips, ENV, 5)
    fr = DeferredFrame(ctx, TileSpec(0, 0, W, H, W, H, 0), g_host, buf[:n], lut, LUT, env, ENV, 5, sky=(sky, ENV, sky_mips))
    fr.set_meshes(v, i, d)
    for sun_args, want_hdr, want_ldr in ((None, hdr_off, ldr_off), (dict(map_size=MAP2, pcf=3, bias=BIAS2), hdr_s, ldr_s),
                                         (dict(map_size=MAP, pcf=3, bias=BIAS), hdr_a, ldr_a)):
        if sun_args is None:
            fr.set_sun(None)
        else:
            fr.set_sun(sun_dir, lum, **sun_args)
        fr.set_prev_luminance(0.18)
        fr.render()
        ctx.sync()
        assert np.array_equal(want_hdr, fr.hdr.cpu().view(torch.int16).numpy().view(np.uint16)), sun_args
        assert np.array_equal(want_ldr, fr.ldr_numpy()), sun_args
        if sun_args and sun_args["map_size"] == MAP2:
            assert np.array_equal(shadow2, fr.shadow_map()[0].cpu().numpy())
    assert np.array_equal(shadow, fr.shadow_map()[0].cpu().numpy())
