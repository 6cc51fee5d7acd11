"""pbr_gbuffer_raster on the GPU: bit parity with the numpy restatement (tests/raster_ref.py) and the contract's properties
against independent truths — watertight meshes, culling, draw order, analytic depth / silhouette / normals — plus tiles,
scratch sizes, refusals and whole frames through DeferredFrame.set_meshes."""
import os

import numpy as np
import pytest
import torch

import camera_cases
import common
import raster_ref
from direct12pbrrenderer_amd import scene
from direct12pbrrenderer_amd.api import PbrError
from direct12pbrrenderer_amd.structs import Tile

PLANES = ("A", "B", "C", "depth", "stencil")


def gpu_raster(ctx, g, tile, v, i, d, minimum=False, extra=0, pitch=None):
    pitch = pitch or tile.w
    n = int((d["index_count"] // 3).sum())
    out = {"A": ctx.zeros((tile.h, pitch), torch.int32), "B": ctx.zeros((tile.h, pitch), torch.int32),
           "C": ctx.zeros((tile.h, pitch), torch.int32), "depth": ctx.zeros((tile.h, pitch), torch.float32),
           "stencil": ctx.zeros((tile.h, pitch), torch.uint8)}
    scratch = ctx.alloc_raster_scratch(tile.w, tile.h, n, minimum=minimum, extra=extra)
    ctx.gbuffer_raster(g, tile, ctx.upload(v), len(v), ctx.upload(i), len(i), ctx.upload(d), len(d), n,
                       out["A"], out["B"], out["C"], out["depth"], out["stencil"], pitch, scratch)
    ctx.sync()
    res = {k: t.cpu().numpy()[:, :tile.w] for k, t in out.items()}
    for k in ("A", "B", "C"):
        res[k] = res[k].view(np.uint32)
    return res


def same(a, b):
    for k in PLANES:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k


def safe_albedo(rng, n):
    """albedo values whose decode_gamma is not within 1e-3 of an 8-bit rounding boundary (the oracle's libm pow and the GPU's
    exp2 / log2 agree there: test_gbuffer_encode_vs_oracle)"""
    out = []
    while len(out) < n:
        a = rng.uniform(0.05, 1.0, 3).astype(np.float32)
        v = (a.astype(np.float64) ** 2.2) * 255.0
        if (np.abs(v - np.floor(v) - 0.5) > 1e-3).all():
            out.append(a)
    return out


def view_to_world(g):
    return np.array(g.InvView[:], dtype=np.float64).reshape(4, 4)


def random_scene(w, h, seed, n=240, camera="default"):
    """Triangles in front of the camera (one of camera_cases.CAMERAS; "default" is the reference's), in four draws with their own
    model matrices: ordinary ones, slivers, degenerate ones, off-screen ones, ones that cross the near plane or leave the guard band."""
    rng = np.random.default_rng(seed)
    cam = camera_cases.camera(camera, w, h)
    g = scene.make_global(cam, w, h)
    th = np.tan(float(cam.fov) / 2.0)
    ms = scene.MeshScene()
    albs = safe_albedo(rng, 4)
    per = n // 4
    for k in range(4):
        tris = []
        for t in range(per):
            z = rng.uniform(0.5, 30.0)
            c = np.array([rng.uniform(-1.2, 1.2) * z * th * float(cam.ratio), rng.uniform(-1.2, 1.2) * z * th, z])
            p = c + rng.normal(scale=0.15 * z, size=(3, 3))
            kind = t % 8
            if kind == 1:      # sliver
                p[2] = p[0] + (p[1] - p[0]) * rng.uniform(0.2, 0.8) + rng.normal(scale=1e-3 * z, size=3)
            elif kind == 2:    # degenerate
                p[1] = p[0]
            elif kind == 3:    # crosses the near plane (one vertex behind the camera or just in front of it)
                p[0, 2] = rng.uniform(-3.0, 0.09)
            elif kind == 4:    # off screen
                p[:, 0] += 4.0 * z * th * float(cam.ratio) * np.sign(rng.uniform(-1, 1))
            elif kind == 5:    # beyond the guard band
                p[0, 0] = 400.0 * z * th * float(cam.ratio) * np.sign(rng.uniform(-1, 1))
            tris.append(p)
        pv = np.concatenate(tris)
        world = (view_to_world(g) @ np.c_[pv, np.ones(len(pv))].T).T[:, :3]
        model = scene.model_matrix(rng.uniform(-2, 2, 3), rng.uniform(-180, 180, 3), rng.uniform(0.5, 2.0, 3))
        local = (np.linalg.inv(model.astype(np.float64)) @ np.c_[world, np.ones(len(world))].T).T[:, :3]
        nrm = rng.normal(size=(len(pv), 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        mesh = scene.Mesh(local, nrm, np.arange(len(pv)))
        ms.add(mesh, model, albedo=albs[k], emission=rng.uniform(0, 1.2), roughness=rng.uniform(0, 1), metallic=rng.uniform(0, 1))
    v, i, d = ms.arrays()
    return g, v, i, d


# the cases under the reference's camera keep their ids; the cameras that pitch and roll (camera_cases.py) at the small size
PARITY_CASES = [pytest.param(257, 131, 1, "default", id="257-131-1"), pytest.param(1440, 960, 2, "default", id="1440-960-2")] + \
               [pytest.param(257, 131, 1, name, id=f"257-131-1-{name}") for name in camera_cases.NON_DEFAULT]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,seed,camera", PARITY_CASES)
def test_parity_with_restatement(ctx, orc, w, h, seed, camera):
    """All five planes bit-identical to raster_ref on random scenes (slivers, degenerate, off-screen, near-plane crossing,
    guard-band triangles)."""
    g, v, i, d = random_scene(w, h, seed, camera=camera)
    tile = Tile(0, 0, w, h, w, h)
    got = gpu_raster(ctx, g, tile, v, i, d)
    want = raster_ref.raster(g, tile, v, i, d, orc)
    assert got["stencil"].any() and (got["stencil"] > 1).any()
    same(got, want)


def grid_scene(w, h, floor=False, seed=5):
    """quad_grid faces -z of its plane (its docstring): placed with a rotation so that -z points at the camera, it is front-facing."""
    cam = scene.Camera.reference_default(w, h)
    g = scene.make_global(cam, w, h)
    th = np.tan(float(cam.fov) / 2.0)
    if floor:   # grid y -> view z (from -10 to 50), grid z -> view -y at y = -1 (below the eye): through the near plane and the guard band
        mesh = scene.quad_grid(48, 48, size=(120.0, 60.0), jitter=0.3, seed=seed)
        to_view = np.array([[1, 0, 0, 0], [0, 0, -1, -1], [0, 1, 0, 20], [0, 0, 0, 1]], dtype=np.float64)
    else:       # a jittered grid in the plane z = 6, larger than the view
        mesh = scene.quad_grid(37, 23, size=(2.4 * 6 * th * float(cam.ratio), 2.4 * 6 * th), jitter=0.35, seed=seed)
        to_view = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 6], [0, 0, 0, 1]], dtype=np.float64)
    model = (view_to_world(g) @ to_view).astype(np.float32)
    ms = scene.MeshScene()
    ms.add(mesh, model, albedo=(0.6, 0.6, 0.6), roughness=0.5)
    v, i, d = ms.arrays()
    return g, v, i, d


def reversed_winding(i):
    return i.reshape(-1, 3)[:, ::-1].reshape(-1).copy()


def facing_camera(ctx, g, w, h, v, i, d):
    """the grid as built (front-facing by construction) and with the winding reversed"""
    tile = Tile(0, 0, w, h, w, h)
    return gpu_raster(ctx, g, tile, v, i, d), gpu_raster(ctx, g, tile, v, reversed_winding(i), d)


@pytest.mark.gpu
def test_watertight_grid_and_culling(ctx):
    """A jittered screen-covering quad grid: stencil == 1 on every pixel; reversed winding: every plane keeps its clear value."""
    w, h = 640, 360
    g, v, i, d = grid_scene(w, h)
    front, back = facing_camera(ctx, g, w, h, v, i, d)
    assert (front["stencil"] == 1).all(), int((front["stencil"] != 1).sum())
    assert not back["stencil"].any() and not back["A"].any() and not back["B"].any() and not back["C"].any()
    assert (back["depth"] == 1.0).all()


@pytest.mark.gpu
def test_watertight_floor_through_near_plane(ctx):
    w, h = 640, 360
    g, v, i, d = grid_scene(w, h, floor=True)
    front, _ = facing_camera(ctx, g, w, h, v, i, d)
    st = front["stencil"]
    assert st.max() == 1 and st[-1].all()
    for col in range(w):
        c = st[:, col]
        top = int(np.argmax(c))
        assert c[top:].all() and not c[:top].any(), col


def parallel_quads(w, h, n, back_to_front, equal=False):
    cam = scene.Camera.reference_default(w, h)
    g = scene.make_global(cam, w, h)
    th = np.tan(float(cam.fov) / 2.0)
    ms = scene.MeshScene()
    zs = np.full(n, 5.0) if equal else np.linspace(30.0, 2.0, n)
    if not back_to_front:
        zs = zs[::-1]
    for k, z in enumerate(zs):
        q = scene.quad_grid(1, 1, size=(0.6 * z * th * float(cam.ratio), 0.6 * z * th))
        to_view = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, z], [0, 0, 0, 1]], dtype=np.float64)
        ms.add(q, (view_to_world(g) @ to_view).astype(np.float32), roughness=(k % 250 + 1) / 255.0, metallic=k / (n - 1) if n > 1 else 0.0)
    v, i, d = ms.arrays()
    return g, v, i, d


@pytest.mark.gpu
def test_draw_order(ctx):
    """300 parallel quads back to front: stencil 255 and the nearest (last) quad's material; front to back: stencil 1 and the
    first; two equal-depth draws: the first draw's material."""
    w, h = 320, 180
    tile = Tile(0, 0, w, h, w, h)
    g, v, i, d = parallel_quads(w, h, 300, True)
    out = gpu_raster(ctx, g, tile, v, i, d)
    on = out["stencil"] > 0
    assert on.sum() > 0.25 * w * h * 0.3 and (out["stencil"][on] == 255).all()
    assert ((out["C"][on] & 255) == (299 % 250 + 1)).all() and (((out["C"][on] >> 8) & 255) == 255).all()
    assert not gpu_raster(ctx, g, tile, v, reversed_winding(i), d)["stencil"].any()
    g, v, i, d = parallel_quads(w, h, 300, False)
    out = gpu_raster(ctx, g, tile, v, i, d)
    on = out["stencil"] > 0
    assert on.any() and (out["stencil"][on] == 1).all() and ((out["C"][on] & 255) == 1).all() and (((out["C"][on] >> 8) & 255) == 0).all()
    g, v, i, d = parallel_quads(w, h, 2, True, equal=True)
    out = gpu_raster(ctx, g, tile, v, i, d)
    on = out["stencil"] > 0
    assert on.any() and (out["stencil"][on] == 1).all() and ((out["C"][on] & 255) == 1).all()


@pytest.mark.gpu
def test_depth_of_slanted_quad_within_2_ulp(ctx):
    """z / w of a large slanted quad against a float64 evaluation: the vertex stage's clip coordinates (float32, as the
    pipeline hands them on), projected, snapped and interpolated in float64."""
    w, h = 1440, 960
    cam = scene.Camera.reference_default(w, h)
    g = scene.make_global(cam, w, h)
    th = np.tan(float(cam.fov) / 2.0)
    # corners in view space (x right, y up), z from 4 (left) to 6 (right), well beyond the view: two triangles, screen-covering
    xs, ys = 1.6 * 6 * th * float(cam.ratio), 1.6 * 6 * th
    pv = np.array([[-xs, ys, 4.0], [xs, ys, 6.0], [xs, -ys, 6.0], [-xs, -ys, 4.0]])
    world = (view_to_world(g) @ np.c_[pv, np.ones(4)].T).T[:, :3]
    ms = scene.MeshScene()
    ms.add(scene.Mesh(world, [(0, 0, 1)] * 4, [0, 1, 2, 0, 2, 3]), np.eye(4, dtype=np.float32))
    v, i, d = ms.arrays()
    tile = Tile(0, 0, w, h, w, h)
    out = gpu_raster(ctx, g, tile, v, i, d)   # TL, TR, BR / TL, BR, BL: clockwise as the camera sees them, i.e. front-facing
    assert (out["stencil"] == 1).all()
    clip, _ = raster_ref.vertex_stage(g, d[0], v["position"], v["normal"])
    c = clip.astype(np.float64)
    sx = np.rint((c[:, 0] / c[:, 3] + 1.0) * (w / 2) * 256.0) / 256.0
    sy = np.rint((1.0 - c[:, 1] / c[:, 3]) * (h / 2) * 256.0) / 256.0
    sz = c[:, 2] / c[:, 3]
    yy, xx = np.mgrid[0:h, 0:w] + 0.5
    want = np.zeros((h, w))
    tri = i.reshape(-1, 3)
    done = np.zeros((h, w), bool)
    for a, b, cc in tri:
        # barycentrics of the pixel centre in the snapped screen triangle (float64)
        den = (sx[b] - sx[a]) * (sy[cc] - sy[a]) - (sy[b] - sy[a]) * (sx[cc] - sx[a])
        l1 = ((xx - sx[a]) * (sy[cc] - sy[a]) - (yy - sy[a]) * (sx[cc] - sx[a])) / den
        l2 = ((sx[b] - sx[a]) * (yy - sy[a]) - (sy[b] - sy[a]) * (xx - sx[a])) / den
        inside = (l1 >= -1e-9) & (l2 >= -1e-9) & (l1 + l2 <= 1 + 1e-9) & ~done
        want[inside] = (sz[a] + l1 * (sz[b] - sz[a]) + l2 * (sz[cc] - sz[a]))[inside]
        done |= inside
    assert done.all()
    got = out["depth"].astype(np.float64)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(got - want) / ulp
    assert err.max() <= 2.0, err.max()


@pytest.mark.gpu
def test_sphere_silhouette_and_normals(ctx):
    """A fine UV sphere on the optical axis: pixels inside the silhouette of its inscribed sphere are covered, pixels outside
    its circumscribed sphere are not, and the encoded normal stays within the facet angle of the analytic one."""
    w, h = 640, 480
    cam = scene.Camera.reference_default(w, h)
    g = scene.make_global(cam, w, h)
    n_lat, n_lon, r, D = 64, 128, 1.0, 5.0
    mesh = scene.uv_sphere(n_lat, n_lon, r)
    to_view = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, D], [0, 0, 0, 1]], dtype=np.float64)
    model = (view_to_world(g) @ to_view).astype(np.float32)
    ms = scene.MeshScene()
    ms.add(mesh, model, roughness=0.5)
    v, i, d = ms.arrays()
    out = gpu_raster(ctx, g, Tile(0, 0, w, h, w, h), v, i, d)
    # uv_sphere's triangles face outwards (its docstring): as built the camera sees the near hemisphere; reversed, the far one
    back = gpu_raster(ctx, g, Tile(0, 0, w, h, w, h), v, reversed_winding(i), d)
    both = (out["stencil"] > 0) & (back["stencil"] > 0)
    assert both.sum() > 0.9 * (out["stencil"] > 0).sum() and (back["depth"][both] > out["depth"][both]).all()
    facet = max(np.pi / n_lat, 2 * np.pi / n_lon)
    r_in = r * np.cos(facet)
    f = (h / 2) / np.tan(float(cam.fov) / 2.0)
    yy, xx = np.mgrid[0:h, 0:w] + 0.5
    rho = np.hypot(xx - w / 2, yy - h / 2)

    def sil(rad):
        return f * rad / np.sqrt(D * D - rad * rad)
    cov = out["stencil"] > 0
    assert cov[rho <= sil(r_in) - 1.0].all()
    assert not cov[rho >= sil(r) + 1.0].any()
    # analytic normal (view space) at the ray / sphere hit, then to world space (the camera's rotation)
    dx, dy = (xx - w / 2) / f, -(yy - h / 2) / f
    dvec = np.stack([dx, dy, np.ones_like(dx)], -1)
    dvec /= np.linalg.norm(dvec, axis=-1, keepdims=True)
    b = dvec[..., 2] * D
    disc = b * b - (D * D - r * r)
    tt = b - np.sqrt(np.maximum(disc, 0))
    nv = dvec * tt[..., None] - np.array([0, 0, D])
    nw = nv @ view_to_world(g)[:3, :3].T
    nw /= np.linalg.norm(nw, axis=-1, keepdims=True)
    bb = out["B"]
    ex, ey = (bb & 255) / 255.0 * 2 - 1, ((bb >> 8) & 255) / 255.0 * 2 - 1
    nz = 1 - np.abs(ex) - np.abs(ey)
    fx = np.where(nz < 0, (1 - np.abs(ey)) * np.where(ex < 0, -1, 1), ex)
    fy = np.where(nz < 0, (1 - np.abs(ex)) * np.where(ey < 0, -1, 1), ey)
    n_dec = np.stack([fx, fy, nz], -1)
    n_dec /= np.linalg.norm(n_dec, axis=-1, keepdims=True)
    sel = cov & (rho <= sil(r_in) - 1.0)
    ang = np.arccos(np.clip((n_dec[sel] * nw[sel]).sum(-1), -1, 1))
    assert ang.max() <= facet + np.radians(1.5), np.degrees(ang.max())


@pytest.mark.gpu
def test_tiles_match_frame(ctx):
    w, h = 257, 131
    g, v, i, d = random_scene(w, h, 7)
    whole = gpu_raster(ctx, g, Tile(0, 0, w, h, w, h), v, i, d)
    for x0, y0, tw, th in [(0, 0, 64, 64), (37, 19, 101, 53), (255, 130, 2, 1), (16, 16, 241, 115), (3, 97, 250, 34)]:
        part = gpu_raster(ctx, g, Tile(x0, y0, tw, th, w, h), v, i, d, pitch=tw + 5)
        same(part, {k: a[y0:y0 + th, x0:x0 + tw] for k, a in whole.items()})


@pytest.mark.gpu
def test_scratch_sizes_and_repeat(ctx):
    """The minimum scratch (every bin walks all triangles), a pool that holds part of the lists, and the recommended size give
    the same bits; so do two runs."""
    w, h = 640, 360
    g, v, i, d = random_scene(w, h, 11, n=400)
    tile = Tile(0, 0, w, h, w, h)
    rec = gpu_raster(ctx, g, tile, v, i, d)
    same(rec, gpu_raster(ctx, g, tile, v, i, d))
    same(rec, gpu_raster(ctx, g, tile, v, i, d, minimum=True))
    same(rec, gpu_raster(ctx, g, tile, v, i, d, minimum=True, extra=4096))


@pytest.mark.gpu
def test_refusals_enqueue_nothing(ctx):
    w, h = 64, 48
    g, v, i, d = random_scene(w, h, 3, n=40)
    n = int((d["index_count"] // 3).sum())
    dv, di, dd = ctx.upload(v), ctx.upload(i), ctx.upload(d)
    planes = [ctx.empty((h, w), torch.int32).fill_(0x5A5A5A5A) for _ in range(3)] + \
             [ctx.empty((h, w), torch.float32).fill_(-7.0), ctx.empty((h, w), torch.uint8).fill_(0xA5)]
    scratch = ctx.alloc_raster_scratch(w, h, n)
    tile = Tile(0, 0, w, h, w, h)
    ok = dict(g=g, tile=tile, vertices=dv, n_vertices=len(v), indices=di, n_indices=len(i), draws=dd, n_draws=len(d), max_triangles=n,
              A=planes[0], B=planes[1], Cc=planes[2], depth=planes[3], stencil=planes[4], pitch=w, scratch=scratch)
    bad = [dict(vertices=0), dict(stencil=0), dict(n_indices=0), dict(n_draws=0), dict(max_triangles=0), dict(pitch=w - 1),
           dict(tile=Tile(10, 0, w, h, w, h)), dict(tile=Tile(0, 0, w, h, 9000, h)), dict(n_draws=70000),
           dict(max_triangles=(1 << 22) + 1), dict(scratch_bytes=ctx.raster_scratch_bytes(w, h, n, minimum=True) - 1)]
    for b in bad:
        args = dict(ok, **b)
        with pytest.raises(PbrError, match="pbr_gbuffer_raster"):
            ctx.gbuffer_raster(**args)
    ctx.sync()
    assert all((p.cpu().numpy().view(np.uint32) == 0x5A5A5A5A).all() for p in planes[:3])
    assert (planes[3].cpu().numpy() == -7.0).all() and (planes[4].cpu().numpy() == 0xA5).all()


def reference_scene():
    """main.json's 33 constant-material models (tests/golden/sphere_grid.npz) and its 8 lights"""
    fx = np.load(os.path.join(common.ROOT, "tests", "golden", "sphere_grid.npz"))
    (v, i, d), names = scene.reference_models(fx)
    rec = common.reference_scene_lights()
    lights = np.concatenate([scene.make_lights(rec["translation"][j], rec["color"][j], rec["radius"][j], rec["intensity"][j])
                             for j in range(len(rec["radius"]))])
    return fx, v, i, d, names, lights


def dev_half(ctx, a):
    return ctx.upload(np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)).view(torch.float16)


@pytest.mark.gpu
def test_frame_from_meshes(ctx, orc):
    """The reference scene's sphere grid and light impostors at 1440x960 through DeferredFrame.set_meshes (reference camera,
    main.json's 8 lights, the small IBL): HDR and LDR bit-identical to a frame fed the same planes through upload_gbuffer; the
    shade of those planes meets the oracle criterion (smoke()'s); every visible sphere centre carries its roughness / metallic
    codes, every visible impostor emission 255."""
    from direct12pbrrenderer_amd.pipeline import DeferredFrame, TileSpec
    w, h = 1440, 960
    sky, env, lut, sh = common.small_ibl(orc)
    cam = scene.Camera.reference_default(w, h)
    g = scene.make_global(cam, w, h, sh_pack=sh)
    fx, v, i, d, names, lights = reference_scene()

    def frame():
        return DeferredFrame(ctx, TileSpec(0, 0, w, h, w, h, 0), g, lights, dev_half(ctx, lut), lut.shape[0], dev_half(ctx, env),
                             common.ENV_SIZE, common.ENV_MIPS)
    a = frame()
    a.set_meshes(v, i, d)
    a.set_prev_luminance(0.18)
    a.render()
    ctx.sync()
    planes = {k: t.cpu().numpy() for k, t in a.gb.items()}
    for k in ("A", "B", "C"):
        planes[k] = planes[k].view(np.uint32)
    on = planes["stencil"] > 0
    assert on.mean() > 0.01
    b = frame()
    b.upload_gbuffer(planes)
    b.set_prev_luminance(0.18)
    b.render()
    ctx.sync()
    assert np.array_equal(a.hdr.cpu().view(torch.int16).numpy(), b.hdr.cpu().view(torch.int16).numpy())
    assert np.array_equal(a.ldr_numpy(), b.ldr_numpy())

    # the shade of the rasterized planes against the float64 evaluation of the reference's formulas, on the covered box
    ys, xs = np.nonzero(on)
    x0, y0, x1, y1 = int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1
    tile = Tile(x0, y0, x1 - x0, y1 - y0, w, h)
    crop = {k: np.ascontiguousarray(p[y0:y1, x0:x1]) for k, p in planes.items()}
    cl = orc.cluster_build(g)
    orc.cluster_cull(g, lights, cl)
    _, hdr32 = orc.deferred_shade(g, tile, crop, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights, want_f32=True)
    lo, hi, flags = orc.deferred_shade_f64(g, tile, crop, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights)
    gb_dev = {k: ctx.upload(p) for k, p in crop.items()}
    out32 = ctx.zeros((tile.h, tile.w, 4), torch.float32)
    ctx.deferred_shade_f32(g, tile, gb_dev, tile.w, a.lut, a.lut_res, a.env, a.env_size, a.env_mips, a.clusters, a.lights, a.n_lights,
                           out32, tile.w)
    ctx.sync()
    ok = (flags == 0) & (crop["stencil"] > 0)
    assert ok.sum() > 0.9 * (crop["stencil"] > 0).sum()
    s32 = float(np.abs(hi[ok]).max())
    d_gpu, d_orc = orc.truth_distance(out32.cpu().numpy(), lo, hi)[ok], orc.truth_distance(hdr32, lo, hi)[ok]
    worst = float((d_gpu / (1e-4 * s32 + 4.0 * d_orc)).max())
    assert worst <= 1.0, worst

    # material codes at the projected centres of the models the pixel shows (its depth between the sphere's front and centre)
    view = np.array(g.View[:], np.float64).reshape(4, 4)
    proj = np.array(g.Projection[:], np.float64).reshape(4, 4)
    seen_grid = seen_imp = 0
    for k, name in enumerate(names):
        tr = fx["trs"][k]
        c, rad = tr[:3].astype(np.float64), float(tr[6]) * 1.0    # the mesh is the unit sphere (its bound: +-1)
        clip = proj @ view @ np.array([*c, 1.0])
        if clip[3] <= 0:
            continue
        x, y = (clip[0] / clip[3] + 1) * w / 2, (1 - clip[1] / clip[3]) * h / 2
        if not (2 <= x < w - 2 and 2 <= y < h - 2):
            continue
        px, py = int(x), int(y)
        zv = (view @ np.array([*c, 1.0]))[2]
        near, far = (proj[2, 2] + proj[2, 3] / z for z in (zv - 1.01 * rad, zv))
        if planes["stencil"][py, px] == 0 or not (near <= planes["depth"][py, px] <= far):
            continue
        mat = fx["material"][k]
        if mat[3] > 0:
            seen_imp += 1
            assert planes["A"][py, px] >> 24 == 255, name
        else:
            seen_grid += 1
            code = (int(np.floor(mat[4] * 255 + 0.5)), int(np.floor(mat[5] * 255 + 0.5)), 0)
            got = planes["C"][py, px]
            assert (got & 255, (got >> 8) & 255, (got >> 16) & 255) == code, name
    # the reference camera sees part of the grid (it stands close in front of it) and all eight impostors
    assert seen_grid >= 5 and seen_imp >= 1, (seen_grid, seen_imp)


@pytest.mark.gpu
def test_host_graph_frame_from_meshes(ctx):
    """pbrh_set_meshes: the C++ pass graph rasterizes the same models in GBufferPass; its G-buffer, HDR and LDR are bit-identical to
    a DeferredFrame of the same meshes, camera, lights (the host's light buffer) and IBL, and the pass order is the reference's."""
    import ctypes as C
    from direct12pbrrenderer_amd import synth
    from direct12pbrrenderer_amd.host import HostRenderer
    from direct12pbrrenderer_amd.pipeline import DeferredFrame, TileSpec
    from direct12pbrrenderer_amd.structs import LIGHT_DTYPE, Global
    W, H, ENV, LUT = 1440, 960, 32, 64
    _, v, i, d, _, lights = reference_scene()
    r = HostRenderer(0, W, H, ENV, LUT)
    try:
        sky_np = synth.env_cube(ENV)
        r.set_skybox(sky_np, ENV)
        r.set_lights(lights)
        r.set_meshes(v, i, d)
        r.set_initial_luminance(0.18)
        r.render(1.0 / 60.0)
        got, want = C.create_string_buffer(512), C.create_string_buffer(512)
        assert r.lib.pbrh_execution_order(r.h, got, 512) == 0 and r.lib.pbrh_dry_run_execution_order(W, H, want, 512) == 0
        assert got.value == want.value and got.value.startswith(b"PreFilterEnvMap")
        planes = {k: r.read(n, (H, W), np.uint32) for k, n in (("A", "GBufferA"), ("B", "GBufferB"), ("C", "GBufferC"))}
        hdr1 = r.read("DeferredShadingRT", (H, W, 4), np.float16)
        ldr1 = r.read("ToneMappedTexture", (H, W), np.uint32)
        g_host = Global()
        assert r.lib.pbrh_get_global(r.h, C.byref(g_host)) == 0
        packed = np.ascontiguousarray(np.concatenate([lights["Position"], lights["Color"], lights["Radius"][:, None],
                                                      lights["Intensity"][:, None]], axis=1), dtype=np.float32)
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
    env = ctx.prefilter_env_dispatches(sky, ENV, sky_mips, ENV, 5)
    fr = DeferredFrame(ctx, TileSpec(0, 0, W, H, W, H, 0), g_host, buf[:n], lut, LUT, env, ENV, 5, sky=(sky, ENV, sky_mips))
    fr.set_meshes(v, i, d)
    fr.set_prev_luminance(0.18)
    fr.render()
    ctx.sync()
    for k in ("A", "B", "C"):
        assert np.array_equal(planes[k], fr.gb[k].cpu().numpy().view(np.uint32)), k
    assert (planes["A"] != 0).any()
    assert np.array_equal(hdr1.view(np.uint16), fr.hdr.cpu().view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(ldr1, fr.ldr_numpy())
