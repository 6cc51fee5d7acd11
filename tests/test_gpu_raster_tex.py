"""pbr_gbuffer_raster with maps on the GPU: parity with the numpy restatement (tests/raster_tex_ref.py) on random textured scenes,
and the sampler's contract against independent truths — no maps equals pbr_gbuffer_raster, mip level selection, wrap
periodicity, an analytic normal-map frame, the C channels — plus tiles, scratch sizes and refusals."""
import numpy as np
import pytest
import torch

import raster_tex_ref
from direct12pbrrenderer_amd import scene
from direct12pbrrenderer_amd.api import PbrError
from direct12pbrrenderer_amd.structs import (NO_MAP, TEX_B8G8R8A8_UNORM, TEX_B8G8R8A8_UNORM_SRGB, TEX_R8_UNORM, TEX_R8G8B8A8_UNORM,
                                             Texture2D, Tile)
from test_gpu_raster import PARITY_CASES, PLANES, gpu_raster, random_scene, same, view_to_world



def upload_textures(ctx, texs):
    keep, descs = [], []
    for t in texs:
        dev, desc = ctx.upload_texture(scene.pack_chain(t["levels"]), t["width"], t["height"], t["mips"], t["format"])
        keep.append(dev)
        descs.append(desc)
    return keep, descs


def gpu_raster_tex(ctx, g, tile, v, i, d, maps, texs, minimum=False, extra=0, descs=None):
    n = int((d["index_count"] // 3).sum())
    out = {"A": ctx.zeros((tile.h, tile.w), torch.int32), "B": ctx.zeros((tile.h, tile.w), torch.int32),
           "C": ctx.zeros((tile.h, tile.w), torch.int32), "depth": ctx.zeros((tile.h, tile.w), torch.float32),
           "stencil": ctx.zeros((tile.h, tile.w), torch.uint8)}
    keep, dd = upload_textures(ctx, texs)
    scratch = ctx.alloc_textured_raster_scratch(tile.w, tile.h, n, minimum=minimum, extra=extra)
    ctx.gbuffer_raster_textured(g, tile, ctx.upload(v), len(v), ctx.upload(i), len(i), ctx.upload(d), len(d), n, out["A"], out["B"],
                                out["C"], out["depth"], out["stencil"], tile.w, scratch, ctx.upload(maps), dd if descs is None else descs)
    ctx.sync()
    res = {k: t.cpu().numpy() for k, t in out.items()}
    for k in ("A", "B", "C"):
        res[k] = res[k].view(np.uint32)
    del keep
    return res


def random_texture(rng, w, h, fmt, mips=None):
    ch = 1 if fmt == TEX_R8_UNORM else 4
    lv0 = rng.integers(0, 256, (h, w, ch) if ch == 4 else (h, w), dtype=np.uint8)
    return raster_tex_ref.texture_dict(scene.mip_chain(lv0, mips), fmt)


def add_tangents_uvs(rng, v, uv_scale):
    """random unit tangents and uv spread far outside [0, 1]"""
    t = rng.normal(size=(len(v), 3))
    v["tangent"] = (t / np.linalg.norm(t, axis=1, keepdims=True)).astype(np.float32)
    v["uv"] = rng.uniform(-uv_scale, uv_scale, (len(v), 2)).astype(np.float32)


def textured_scene(w, h, seed, camera="default"):
    """raster_test's random scene (slivers, near-plane crossings, guard band) with tangents, uvs, and textures of every format,
    square, non-square and non-power-of-two, some with partial chains; draw 0 takes constants only, the others mixes of maps."""
    g, v, i, d = random_scene(w, h, seed, camera=camera)
    rng = np.random.default_rng(seed + 100)
    add_tangents_uvs(rng, v, 6.0)
    texs = [random_texture(rng, 64, 64, TEX_R8G8B8A8_UNORM), random_texture(rng, 37, 21, TEX_B8G8R8A8_UNORM_SRGB),
            random_texture(rng, 128, 32, TEX_B8G8R8A8_UNORM, mips=4), random_texture(rng, 19, 50, TEX_R8_UNORM),
            random_texture(rng, 16, 16, TEX_R8_UNORM, mips=1), random_texture(rng, 256, 96, TEX_B8G8R8A8_UNORM_SRGB)]
    maps = np.full(len(d), NO_MAP, dtype=scene.DRAW_MAPS_DTYPE)
    maps[1] = (0, 1, 3, 4, 3)
    maps[2] = (5, NO_MAP, 4, NO_MAP, 3)
    maps[3] = (2, 2, NO_MAP, 3, 4)
    return g, v, i, d, maps, texs


def compare(got, want, what=""):
    """depth / stencil / coverage bit-identical; A, B, C within one UNORM8 step, identical on >= 99.9 % of covered pixels"""
    for k in ("depth", "stencil"):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k)
    cov = want["stencil"] > 0
    counts = {}
    for k in ("A", "B", "C"):
        a = got[k].view(np.uint8).reshape(*got[k].shape, 4).astype(np.int32)
        b = want[k].view(np.uint8).reshape(*want[k].shape, 4).astype(np.int32)
        diff = np.abs(a - b).max(axis=-1)
        assert (diff[~cov] == 0).all(), (what, k, "outside coverage")
        assert diff.max() <= 1, (what, k, int(diff.max()))
        counts[k] = int((diff[cov] != 0).sum())
        assert counts[k] <= 1e-3 * cov.sum(), (what, k, counts[k], int(cov.sum()))
    print(f"{what}: {int(cov.sum())} covered pixels, differing by one step: {counts}")
    return counts


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,seed,camera", PARITY_CASES)
def test_parity_with_restatement(ctx, orc, w, h, seed, camera):
    g, v, i, d, maps, texs = textured_scene(w, h, seed, camera)
    tile = Tile(0, 0, w, h, w, h)
    got = gpu_raster_tex(ctx, g, tile, v, i, d, maps, texs)
    want = raster_tex_ref.raster_textured(g, tile, v, i, d, maps, texs, orc)
    assert (got["stencil"] > 1).any()
    cm = got["C"].view(np.uint8).reshape(h, w, 4)
    assert (cm[..., 2] > 0).sum() > 100        # AO from maps landed
    compare(got, want, f"parity {w}x{h}")


@pytest.mark.gpu
def test_no_maps_equals_constant_raster(ctx):
    w, h = 257, 131
    g, v, i, d, maps, texs = textured_scene(w, h, 3)
    maps[:] = NO_MAP
    tile = Tile(0, 0, w, h, w, h)
    same(gpu_raster_tex(ctx, g, tile, v, i, d, maps, texs), gpu_raster(ctx, g, tile, v, i, d))


def screen_quad(w, h, uv_per_px, uv0=(0.0, 0.0), z=4.0, tangent=(1.0, 0.0, 0.0)):
    """A quad facing the camera covering the whole w x h frame, uv = uv0 + uv_per_px * (pixel position), normal towards the
    camera, tangent as given (world space, the model is the camera frame)."""
    cam = scene.Camera.reference_default(w, h)
    g = scene.make_global(cam, w, h)
    th = np.tan(float(cam.fov) / 2.0)
    hw, hh = 1.2 * z * th * float(cam.ratio), 1.2 * z * th
    p = np.array([[-hw, hh, z], [hw, hh, z], [hw, -hh, z], [-hw, -hh, z]])
    # the corners' pixel positions through the camera's projection (the model is the camera frame)
    clip = (np.array(g.Projection[:], np.float64).reshape(4, 4) @ np.c_[p, np.ones(4)].T).T
    sx = (clip[:, 0] / clip[:, 3] + 1.0) * w / 2
    sy = (1.0 - clip[:, 1] / clip[:, 3]) * h / 2
    uv = np.stack([uv0[0] + uv_per_px * sx, uv0[1] + uv_per_px * sy], axis=1)
    tris = scene._orient(p, np.array([[0, 1, 2], [0, 2, 3]]), lambda q: np.broadcast_to([0.0, 0.0, -1.0], (len(q), 3)))
    mesh = scene.Mesh(p, np.broadcast_to([0.0, 0.0, -1.0], (4, 3)), tris, tangents=np.broadcast_to(tangent, (4, 3)), uvs=uv)
    model = view_to_world(g).astype(np.float32)
    return g, mesh, model


def level_texture(size, colours, fmt=TEX_R8G8B8A8_UNORM):
    """a square texture whose level l is the constant colour colours[l] (RGBA bytes)"""
    levels = [np.broadcast_to(np.asarray(colours[l], np.uint8), (size >> l, size >> l, 4)).copy() for l in range(len(colours))]
    return raster_tex_ref.texture_dict(levels, fmt)


def draw_one(ctx, w, h, g, mesh, model, maps, texs, albedo=(0.5, 0.5, 0.5), roughness=0.5, metallic=0.0):
    ms = scene.MeshScene()
    ms.add(mesh, model, albedo=albedo, roughness=roughness, metallic=metallic, maps=maps)
    v, i, d = ms.arrays()
    return gpu_raster_tex(ctx, g, Tile(0, 0, w, h, w, h), v, i, d, ms.maps(), texs), (v, i, d, ms.maps())


@pytest.mark.gpu
def test_mip_level_selection(ctx):
    """A screen-aligned quad at 2^k texels per pixel on a texture whose levels are distinct constants reads level k's value
    exactly; at 2^(k + 1/2) the midpoint of levels k and k + 1 (one step).  Read through the roughness channel (no gamma)."""
    w, h, size = 96, 64, 256
    reds = [16 * l + 8 + (l % 2) * 100 for l in range(9)]
    tex = level_texture(size, [(r, 0, 0, 255) for r in reds])
    for k in range(6):
        for half in (False, True):
            ppx = 2.0 ** (k + (0.5 if half else 0.0)) / size
            g, mesh, model = screen_quad(w, h, ppx, uv0=(0.3, 0.7))
            got, _ = draw_one(ctx, w, h, g, mesh, model, {"roughness": 0}, [tex])
            cov = got["stencil"] > 0
            assert cov.all()
            r = (got["C"] & 255).astype(np.int32)
            want = reds[k] if not half else (reds[k] + reds[k + 1]) / 2.0
            assert np.abs(r - want).max() <= (0.5 if half else 0), (k, half, np.unique(r))


@pytest.mark.gpu
def test_wrap_periodicity(ctx):
    """uv shifted by whole periods (here +3, -5) gives the same planes"""
    w, h = 128, 96
    rng = np.random.default_rng(7)
    tex = random_texture(rng, 32, 32, TEX_B8G8R8A8_UNORM)
    outs = []
    for off in (0.0, 3.0, -5.0):
        g, mesh, model = screen_quad(w, h, 0.37 / 32, uv0=(0.25 + off, 0.125 - off))
        got, _ = draw_one(ctx, w, h, g, mesh, model, {"albedo": 0, "roughness": 0}, [tex])
        outs.append(got)
    cov = outs[0]["stencil"] > 0
    assert cov.mean() > 0.99
    for o in outs[1:]:
        for k in ("A", "C"):
            d = np.abs(o[k].view(np.uint8).astype(np.int32) - outs[0][k].view(np.uint8).astype(np.int32))
            # uv = uv0 + s x is rounded differently at another offset: allow one step on a few pixels
            assert d.max() <= 1 and (d != 0).mean() < 0.02, k


@pytest.mark.gpu
def test_tilted_normal_map(ctx, orc):
    """A constant normal map (tangent-space direction ts) on a camera-facing quad: B = the octahedral code of ts.x t + ts.y b +
    ts.z n, with n = (0, 0, -1) and t = (1, 0, 0) in view space, b = n x t."""
    w, h = 64, 48
    rgb = (200, 90, 230)
    tex = level_texture(8, [(*rgb, 255)] * 4)
    g, mesh, model = screen_quad(w, h, 1.0 / 64, tangent=(1.0, 0.0, 0.0))
    # the model is the camera frame: tangent (1, 0, 0) and normal (0, 0, -1) of the mesh are view-space directions
    got, _ = draw_one(ctx, w, h, g, mesh, model, {"normal": 0}, [tex])
    ts = np.array(rgb, np.float64) / 255.0 * 2 - 1
    Vinv = view_to_world(g)[:3, :3]
    n_v, t_v = np.array([0.0, 0.0, -1.0]), np.array([1.0, 0.0, 0.0])
    b_v = np.cross(n_v, t_v)
    nw = Vinv @ (ts[0] * t_v + ts[1] * b_v + ts[2] * n_v)
    nw /= np.linalg.norm(nw)
    m1 = np.zeros((1, 1, 4), np.float32)
    m1[0, 0, :3] = nw
    _, Bw, _ = orc.gbuffer_encode(np.zeros((1, 1, 4), np.float32), m1, np.zeros((1, 1, 4), np.float32))
    B = got["B"].view(np.uint8).reshape(h, w, 4)[..., :2].astype(np.int32)
    want = np.frombuffer(Bw.tobytes(), np.uint8)[:2].astype(np.int32)
    assert (got["stencil"] > 0).all()
    assert np.abs(B - want).max() <= 1


@pytest.mark.gpu
def test_maps_land_in_their_channels(ctx):
    """R8 maps of three constants -> C = (roughness, metallic, AO); a BGRA albedo map -> A's red is the texel's red"""
    w, h = 64, 48
    r8 = lambda c: raster_tex_ref.texture_dict([np.full((4 >> l, 4 >> l), c, np.uint8) for l in range(3)], TEX_R8_UNORM)
    bgra = raster_tex_ref.texture_dict([np.broadcast_to(np.array([10, 20, 255, 7], np.uint8), (4, 4, 4)).copy()], TEX_B8G8R8A8_UNORM)
    g, mesh, model = screen_quad(w, h, 1.0 / 64)
    got, _ = draw_one(ctx, w, h, g, mesh, model, {"roughness": 0, "metallic": 1, "ao": 2, "albedo": 3},
                      [r8(51), r8(102), r8(204), bgra], roughness=0.9, metallic=0.9)
    Cb = got["C"].view(np.uint8).reshape(h, w, 4)
    assert (Cb[..., 0] == 51).all() and (Cb[..., 1] == 102).all() and (Cb[..., 2] == 204).all()
    Ab = got["A"].view(np.uint8).reshape(h, w, 4)
    assert (Ab[..., 0] == 255).all() and (Ab[..., 2] < Ab[..., 1]).all()    # decode_gamma(1) = 1; blue < green


@pytest.mark.gpu
def test_tiles_and_scratch_sizes(ctx):
    """tiles with odd x0 / y0 are bit-identical to the frame; every scratch size from the minimum up gives the same bits"""
    w, h = 257, 131
    g, v, i, d, maps, texs = textured_scene(w, h, 4)
    full = gpu_raster_tex(ctx, g, Tile(0, 0, w, h, w, h), v, i, d, maps, texs)
    for x0, y0, tw, th in ((1, 3, 101, 77), (33, 17, 224, 114), (129, 65, 64, 33)):
        got = gpu_raster_tex(ctx, g, Tile(x0, y0, tw, th, w, h), v, i, d, maps, texs)
        for k in PLANES:
            assert np.array_equal(got[k].view(np.uint8), full[k][y0:y0 + th, x0:x0 + tw].view(np.uint8)), (x0, y0, k)
    n = int((d["index_count"] // 3).sum())
    lo, rec = ctx.textured_raster_scratch_bytes(w, h, n, minimum=True), ctx.textured_raster_scratch_bytes(w, h, n)
    for extra in (0, 4 * 37, (rec - lo) // 2, rec - lo):
        same(gpu_raster_tex(ctx, g, Tile(0, 0, w, h, w, h), v, i, d, maps, texs, minimum=True, extra=extra), full)


@pytest.mark.gpu
def test_bad_map_index_drops_the_draw(ctx, orc):
    """a draw with a map index >= n_textures is dropped on the device (the restatement agrees)"""
    w, h = 257, 131
    g, v, i, d, maps, texs = textured_scene(w, h, 5)
    maps[2]["metallic"] = len(texs)
    tile = Tile(0, 0, w, h, w, h)
    got = gpu_raster_tex(ctx, g, tile, v, i, d, maps, texs)
    compare(got, raster_tex_ref.raster_textured(g, tile, v, i, d, maps, texs, orc), "bad map index")
    # the same planes as the scene without draw 2's triangles
    maps[2]["metallic"] = NO_MAP
    d2 = d.copy()
    d2["index_count"][2] = 0
    same(got, gpu_raster_tex(ctx, g, tile, v, i, d2, maps, texs))
    assert not np.array_equal(got["stencil"], gpu_raster_tex(ctx, g, tile, v, i, d, maps, texs)["stencil"])


@pytest.mark.gpu
def test_refusals_enqueue_nothing(ctx):
    w, h = 64, 48
    rng = np.random.default_rng(9)
    tex = random_texture(rng, 16, 8, TEX_B8G8R8A8_UNORM)
    g, mesh, model = screen_quad(w, h, 1.0 / 16)
    ms = scene.MeshScene()
    ms.add(mesh, model, maps={"albedo": 0})
    v, i, d = ms.arrays()
    tile = Tile(0, 0, w, h, w, h)
    keep, (good,) = upload_textures(ctx, [tex])
    dev = keep[0]
    base = dev.data_ptr()

    def bad(**kw):
        f = dict(texels=base, width=16, height=8, mip_levels=4, format=TEX_B8G8R8A8_UNORM)
        f.update(kw)
        return Texture2D(f["texels"], f["width"], f["height"], f["mip_levels"], f["format"])

    fmt, size, mips, texels = "unknown texture format", "texture size zero or above", "mip_levels 0 or above", "texels null or not aligned"
    cases = [([bad(format=29)], fmt), ([bad(format=0)], fmt), ([bad(width=0)], size), ([bad(height=0)], size),
             ([bad(width=16385, height=16385)], size), ([bad(mip_levels=0)], mips), ([bad(mip_levels=5)], mips), ([bad(texels=0)], texels),
             ([bad(texels=base + 2)], texels), ([good] * 65, "more textures than")]
    n = 2
    planes = [ctx.zeros((h, w), torch.int32) for _ in range(3)] + [ctx.zeros((h, w), torch.float32), ctx.zeros((h, w), torch.uint8)]
    for p in planes:
        p.fill_(7)
    scratch = ctx.alloc_textured_raster_scratch(w, h, n)
    dv, di, dd, dm = ctx.upload(v), ctx.upload(i), ctx.upload(d), ctx.upload(ms.maps())
    for descs, why in cases:
        with pytest.raises(PbrError, match="pbr_gbuffer_raster: " + why):
            ctx.gbuffer_raster_textured(g, tile, dv, len(v), di, len(i), dd, len(d), n, *planes, w, scratch, dm, descs)
    with pytest.raises(PbrError):        # scratch of the constant raster is below the textured minimum
        small = ctx.alloc_raster_scratch(w, h, n, minimum=True)
        ctx.gbuffer_raster_textured(g, tile, dv, len(v), di, len(i), dd, len(d), n, *planes, w, small, dm, [good])
    with pytest.raises(PbrError):        # no maps
        ctx.gbuffer_raster_textured(g, tile, dv, len(v), di, len(i), dd, len(d), n, *planes, w, scratch, None, [good])
    ctx.sync()
    for p in planes:
        assert (p.cpu().numpy() == 7).all()
    # a valid call still runs
    ctx.gbuffer_raster_textured(g, tile, dv, len(v), di, len(i), dd, len(d), n, *planes, w, scratch, dm, [good])
    ctx.sync()
    assert (planes[4].cpu().numpy() == 1).all()
    # R8 texels need no alignment: a chain at an odd address is accepted and sampled as given
    r8 = raster_tex_ref.texture_dict(scene.mip_chain(np.full((8, 16), 153, np.uint8)), TEX_R8_UNORM)
    buf = ctx.upload(np.concatenate([np.zeros(1, np.uint8), scene.pack_chain(r8["levels"])]))
    odd = Texture2D(buf.data_ptr() + 1, 16, 8, r8["mips"], TEX_R8_UNORM)
    ms2 = scene.MeshScene()
    ms2.add(mesh, model, maps={"roughness": 0})
    ctx.gbuffer_raster_textured(g, tile, dv, len(v), di, len(i), dd, len(d), n, *planes, w, scratch, ctx.upload(ms2.maps()), [odd])
    ctx.sync()
    assert ((planes[2].cpu().numpy() & 255) == 153).all()


@pytest.mark.gpu
def test_deferred_frame_set_meshes_with_maps(ctx):
    """DeferredFrame.set_meshes(..., maps, textures) rasterizes through the textured entry: the same planes as the direct call"""
    from direct12pbrrenderer_amd.pipeline import DeferredFrame, TileSpec
    import common
    w, h = 257, 131
    g, v, i, d, maps, texs = textured_scene(w, h, 6)
    want = gpu_raster_tex(ctx, g, Tile(0, 0, w, h, w, h), v, i, d, maps, texs)
    keep, descs = upload_textures(ctx, texs)
    lut = ctx.zeros((8, 8, 4), torch.float16)
    env = ctx.zeros((common.ENV_SIZE * common.ENV_SIZE * 8 * 4,), torch.float16)
    fr = DeferredFrame(ctx, TileSpec(0, 0, w, h, w, h, 0), g, np.zeros(0, scene.LIGHT_DTYPE), lut, 8, env, common.ENV_SIZE,
                       common.ENV_MIPS)
    fr.set_meshes(v, i, d, maps=maps, textures=list(zip(keep, descs)))
    del keep, descs                 # the frame holds the texture memory
    torch.cuda.empty_cache()
    fr.rasterize()
    ctx.sync()
    got = {k: t.cpu().numpy() for k, t in fr.gb.items()}
    for k in ("A", "B", "C"):
        got[k] = got[k].view(np.uint32)
    same(got, want)


def reference_textured_scene(w, h, orc):
    """main.json's 33 constant-material models and its four textured ones (tests/golden/textured_models.npz), camera, lights, IBL"""
    import os
    import common
    fx = np.load(os.path.join(common.ROOT, "tests", "golden", "sphere_grid.npz"))
    fxt = np.load(os.path.join(common.ROOT, "tests", "golden", "textured_models.npz"))
    ms = scene.MeshScene()
    scene.reference_models(fx, ms)
    texs, names = scene.add_textured_models(ms, fxt)
    v, i, d = ms.arrays()
    rec = common.reference_scene_lights()
    lights = np.concatenate([scene.make_lights(rec["translation"][j], rec["color"][j], rec["radius"][j], rec["intensity"][j])
                             for j in range(len(rec["radius"]))])
    sky, env, lut, sh = common.small_ibl(orc)
    g = scene.make_global(scene.Camera.reference_default(w, h), w, h, sh_pack=sh)
    return g, v, i, d, ms.maps(), texs, lights, lut, env


@pytest.mark.gpu
def test_reference_scene_raster_and_shade(ctx, orc):
    """The reference scene with its hero models at 1440x960: the raster against the restatement, then the shade of the GPU's planes
    against the oracle's shade of the restatement's planes (smoke()'s criterion, on the pixels whose planes agree)."""
    import common
    w, h = 1440, 960
    g, v, i, d, maps, texs, lights, lut, env = reference_textured_scene(w, h, orc)
    tile = Tile(0, 0, w, h, w, h)
    got = gpu_raster_tex(ctx, g, tile, v, i, d, maps, texs)
    want = raster_tex_ref.raster_textured(g, tile, v, i, d, maps, texs, orc)
    compare(got, want, "reference scene")
    # the hero models are on screen: their pixels carry map AO
    ao = (got["C"] >> 16) & 255
    assert (ao > 0).sum() > 1000, int((ao > 0).sum())

    cl = orc.cluster_build(g)
    orc.cluster_cull(g, lights, cl)
    ref = {k: np.ascontiguousarray(want[k]) for k in PLANES}
    _, hdr32 = orc.deferred_shade(g, tile, ref, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights, want_f32=True)
    lo, hi, flags = orc.deferred_shade_f64(g, tile, ref, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights)
    from direct12pbrrenderer_amd.pipeline import DeferredFrame, TileSpec

    def dev_half(a):
        return ctx.upload(np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)).view(torch.float16)
    fr = DeferredFrame(ctx, TileSpec(0, 0, w, h, w, h, 0), g, lights, dev_half(lut), lut.shape[0], dev_half(env), common.ENV_SIZE,
                       common.ENV_MIPS)
    fr.clustered()
    gb_dev = {k: ctx.upload(np.ascontiguousarray(got[k])) for k in PLANES}
    out32 = ctx.zeros((h, w, 4), torch.float32)
    ctx.deferred_shade_f32(g, tile, gb_dev, w, fr.lut, fr.lut_res, fr.env, fr.env_size, fr.env_mips, fr.clusters, fr.lights, fr.n_lights,
                           out32, w)
    ctx.sync()
    agree = np.ones((h, w), bool)
    for k in ("A", "B", "C"):
        agree &= got[k] == want[k]
    cov = want["stencil"] > 0
    ok = (flags == 0) & cov & agree
    assert ok.sum() > 0.9 * cov.sum()
    # the shade bound's domain: roughness >= 48 / 255; the maps also hold lower roughness codes, where the
    # GGX peak amplifies fp32 rounding beyond the bound for the kernel and the fp32 restatement alike
    ok &= (want["C"] & 255) >= 48
    print(f"reference scene shade: {int(ok.sum())} of {int(cov.sum())} covered pixels compared")
    assert ok.sum() > 100000
    s32 = float(np.abs(hi[ok]).max())
    d_gpu, d_orc = orc.truth_distance(out32.cpu().numpy(), lo, hi)[ok], orc.truth_distance(hdr32, lo, hi)[ok]
    worst = float((d_gpu / (1e-4 * s32 + 4.0 * d_orc)).max())
    assert worst <= 1.0, worst


@pytest.mark.gpu
def test_host_graph_textured_meshes(ctx, orc):
    """pbrh_set_textured_meshes: the C++ pass graph's GBufferPass rasterizes the reference scene with its hero models through
    pbr_gbuffer_raster with maps; its G-buffer planes equal the direct C call's with the host's camera."""
    import ctypes as C
    from direct12pbrrenderer_amd import synth
    from direct12pbrrenderer_amd.host import HostRenderer
    from direct12pbrrenderer_amd.structs import Global
    W, H, ENV, LUT = 1440, 960, 32, 64
    _, v, i, d, maps, texs, lights, _, _ = reference_textured_scene(W, H, orc)
    r = HostRenderer(0, W, H, ENV, LUT)
    try:
        r.set_skybox(synth.env_cube(ENV), ENV)
        r.set_lights(lights)
        r.set_textured_meshes(v, i, d, maps, [(scene.pack_chain(t["levels"]), t["width"], t["height"], t["mips"], t["format"])
                                             for t in texs])
        r.set_initial_luminance(0.18)
        r.render(1.0 / 60.0)
        planes = {k: r.read(n, (H, W), np.uint32) for k, n in (("A", "GBufferA"), ("B", "GBufferB"), ("C", "GBufferC"))}
        g_host = Global()
        assert r.lib.pbrh_get_global(r.h, C.byref(g_host)) == 0
    finally:
        r.close()
    want = gpu_raster_tex(ctx, g_host, Tile(0, 0, W, H, W, H), v, i, d, maps, texs)
    for k in ("A", "B", "C"):
        assert np.array_equal(planes[k], want[k]), k
    assert (((planes["C"] >> 16) & 255) > 0).sum() > 1000
