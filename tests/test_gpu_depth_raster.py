"""pbr_depth_raster on the GPU: its depth plane is pbr_gbuffer_raster's, bit for bit — on the cases of tests/raster_cover_truth.py
(where the plane alone also passes the float64 truth's depth conditions), with a bin list longer than the G-buffer chain's 2048, under
triangles that touch every bin, with the draws reversed, with the model cull, on ragged tiles and under the sun's light camera; every
pixel of the tile is written and nothing around it; the refusals enqueue nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import raster_cover_truth as T
import sun_cases as sc
from direct12pbrrenderer_amd import api, scene
from direct12pbrrenderer_amd.api import PbrError
from direct12pbrrenderer_amd.structs import DepthRasterDesc, Tile
from test_gpu_raster import gpu_raster, random_scene
from test_gpu_raster_cull import Buffers, cull_scene
import camera_cases

GUARD_ROWS = 3
SENTINEL = 0x7FC5A5A5       # a quiet NaN no kernel writes


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def equal(a, b):
    return np.array_equal(bits(a), bits(b))


class Target:
    """a depth plane of tile.h rows at `pitch`, filled with the sentinel, inside GUARD_ROWS sentinel rows above and below"""

    def __init__(self, ctx, tile, pitch=None):
        self.ctx, self.tile, self.pitch = ctx, tile, pitch or tile.w
        self.buf = ctx.empty((tile.h + 2 * GUARD_ROWS, self.pitch), torch.int32)
        self.buf.fill_(SENTINEL)
        self.ptr = self.buf.data_ptr() + GUARD_ROWS * self.pitch * 4

    def raw(self):
        self.ctx.sync()
        return self.buf.cpu().numpy().view(np.uint32)

    def untouched(self):
        return bool((self.raw() == SENTINEL).all())

    def depth(self):
        """the tile's depth [h, w]; the guard rows and the columns from w to pitch must hold the sentinel, the tile must not"""
        a = self.raw()
        assert (a[:GUARD_ROWS] == SENTINEL).all() and (a[-GUARD_ROWS:] == SENTINEL).all(), "guard rows written"
        assert (a[GUARD_ROWS:-GUARD_ROWS, self.tile.w:] == SENTINEL).all(), "columns past the tile's width written"
        d = np.ascontiguousarray(a[GUARD_ROWS:-GUARD_ROWS, :self.tile.w])
        assert not (d == SENTINEL).any(), "a pixel of the tile was not written"
        return d.view(np.float32)


def gpu_depth(ctx, g, tile, v, i, d, scratch="recommended", pitch=None, bounds=None, stats=None):
    """pbr_depth_raster into a guarded target; scratch: recommended, minimum, or halfway between the two"""
    n = int((d["index_count"] // 3).sum())
    lo, hi = ctx.depth_raster_scratch_bytes(tile.w, tile.h, n, minimum=True), ctx.depth_raster_scratch_bytes(tile.w, tile.h, n)
    nbytes = {"recommended": hi, "minimum": lo, "halfway": ((lo + hi) // 2) & ~3}[scratch]
    buf = ctx.alloc_depth_raster_scratch(tile.w, tile.h, n)
    t = Target(ctx, tile, pitch)
    ctx.depth_raster(g, tile, ctx.upload(v), len(v), ctx.upload(i), len(i), ctx.upload(d), len(d), n, t.ptr, t.pitch, buf, nbytes,
                     bounds=bounds, stats=stats)
    return t.depth()


def screen_scene(W, H, groups):
    """draws of screen-space triangles under raster_cover_truth.identity_global: groups = [(pts [n, 3, 2] pixels, z [n, 3])], all
    wound front-facing (clockwise on the y-down screen)"""
    ms = scene.MeshScene()
    for pts, z in groups:
        pos = np.zeros((len(pts), 3, 3))
        for t, (p, zz) in enumerate(zip(np.asarray(pts, np.float64), np.asarray(z, np.float64))):
            o = T._wind(p[:, 0], p[:, 1], True)
            pos[t, :, 0], pos[t, :, 1], pos[t, :, 2] = p[o, 0] / (0.5 * W) - 1.0, 1.0 - p[o, 1] / (0.5 * H), zz[o]
        pos = pos.reshape(-1, 3)
        ms.add(scene.Mesh(pos, np.broadcast_to([0.0, 0.0, 1.0], pos.shape), np.arange(len(pos))), np.eye(4, dtype=np.float32),
               roughness=0.5, metallic=0.0)
    return T.identity_global(W, H), ms.arrays()


def small_triangles(rng, W, H, n, radius=(0.8, 2.5)):
    c = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], axis=1)[:, None, :]
    a = rng.uniform(0, 2 * np.pi, (n, 1)) + np.radians([0.0, 120.0, 240.0])[None, :]
    r = rng.uniform(*radius, (n, 1))
    return c + r[..., None] * np.stack([np.cos(a), np.sin(a)], axis=2), rng.uniform(0.02, 0.98, (n, 3))


# ---- 1. the cover cases
@pytest.mark.gpu
@pytest.mark.parametrize("name", T.CASE_NAMES + T.FLOOR_NAMES)
def test_cover_cases(ctx, name):
    case = T.case(name)
    floor = name in T.FLOOR_NAMES
    v, i, d = case.scene()
    want = gpu_raster(ctx, case.g, case.tile, v, i, d, pitch=case.pitch)
    got = gpu_depth(ctx, case.g, case.tile, v, i, d, pitch=case.pitch)
    assert (want["stencil"] > 0).any() and equal(got, want["depth"])
    # the depth plane alone against the float64 truth (the other four planes are the G-buffer call's)
    res = T.check(case.truth, dict(want, depth=got), winners=not floor, what=name)
    print(T.report(name, res))
    if floor:
        assert equal(gpu_depth(ctx, case.g, case.tile, v, i, d, scratch="minimum"), want["depth"])
        assert equal(gpu_depth(ctx, case.g, case.tile, v, i, d, scratch="halfway"), want["depth"])
        tile = Tile(*T.FLOOR_TILE, *case.full)
        whole = want["depth"][tile.y0:tile.y0 + tile.h, tile.x0:tile.x0 + tile.w]
        for scratch in ("recommended", "minimum", "halfway"):
            assert equal(gpu_depth(ctx, case.g, tile, v, i, d, scratch=scratch, pitch=tile.w + 5), whole), scratch


# ---- 2. and 4. one bin with a list longer than the G-buffer chain's cap; the same draws reversed
LONG = 2304


def long_list_scene():
    rng = np.random.default_rng(2304)
    pts, z = small_triangles(rng, 16, 16, LONG)
    # the triangles whose box holds a pixel centre of the target are the one bin's list: longer than the G-buffer chain's 2048
    lo, hi = np.ceil(pts.min(axis=1) - 0.5).clip(0, 15), np.floor(pts.max(axis=1) - 0.5).clip(0, 15)
    assert int((lo <= hi).all(axis=1).sum()) > 2048 + 128
    return screen_scene(16, 16, [(pts[k::4], z[k::4]) for k in range(4)])


@pytest.mark.gpu
def test_a_list_longer_than_2048_in_one_bin(ctx):
    g, (v, i, d) = long_list_scene()
    tile = Tile(0, 0, 16, 16, 16, 16)
    want = gpu_raster(ctx, g, tile, v, i, d)
    assert (want["stencil"] > 0).all() and len(np.unique(want["depth"])) > 200      # every pixel is covered, and the depths differ
    for scratch in ("recommended", "minimum"):
        assert equal(gpu_depth(ctx, g, tile, v, i, d, scratch=scratch), want["depth"]), scratch


@pytest.mark.gpu
def test_order_independence(ctx):
    g, (v, i, d) = long_list_scene()
    tile = Tile(0, 0, 16, 16, 16, 16)
    forward = gpu_depth(ctx, g, tile, v, i, d)
    assert equal(gpu_depth(ctx, g, tile, v, i, d[::-1].copy()), forward)
    assert equal(gpu_depth(ctx, g, tile, v, i, d[::-1].copy(), scratch="minimum"), forward)


# ---- 3. triangles whose box holds every bin
@pytest.mark.gpu
def test_a_triangle_over_every_bin(ctx):
    W, H = 257, 131
    rng = np.random.default_rng(500)
    cover = np.array([[(-9.0, -7.0), (W + 9.0, -7.0), (W + 9.0, H + 7.0)], [(-9.0, -7.0), (W + 9.0, H + 7.0), (-9.0, H + 7.0)]])
    g, (v, i, d) = screen_scene(W, H, [(cover, np.full((2, 3), 0.75)), small_triangles(rng, W, H, 500, radius=(1.5, 9.0))])
    tile = Tile(0, 0, W, H, W, H)
    want = gpu_raster(ctx, g, tile, v, i, d)
    assert (want["stencil"] > 0).all() and (want["depth"] == np.float32(0.75)).any() and (want["depth"] < np.float32(0.75)).any()
    for scratch in ("recommended", "halfway", "minimum"):
        assert equal(gpu_depth(ctx, g, tile, v, i, d, scratch=scratch), want["depth"]), scratch


# ---- 5. the model cull
@pytest.mark.gpu
def test_cull(ctx):
    fw, fh = 70, 45
    g = camera_cases.make_global("default", fw, fh)[1]
    v, i, d, b = cull_scene("first_last", g)
    tile = Tile(0, 0, fw, fh, fw, fh)
    bufs = Buffers(ctx, v, i, d, b)
    plain, _ = bufs.run(g, tile, False)
    _, want_stats = bufs.run(g, tile, True)
    assert want_stats[1] == 2 and (plain["stencil"] > 0).any()       # the first and the last draw are culled
    st = ctx.alloc_cull_stats()
    assert equal(gpu_depth(ctx, g, tile, v, i, d, bounds=bufs.db, stats=st), plain["depth"])
    assert ctx.read_cull_stats(st).astuple() == want_stats
    assert equal(gpu_depth(ctx, g, tile, v, i, d, bounds=bufs.db), plain["depth"])      # stats may be null
    assert equal(gpu_depth(ctx, g, tile, v, i, d), plain["depth"])


# ---- 6. ragged shapes
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1, 1), (17, 16), (200, 37)])
def test_ragged_shapes(ctx, w, h):
    g, v, i, d = random_scene(w, h, 64, n=64, camera="pitch_roll")
    tile = Tile(0, 0, w, h, w, h)
    want = gpu_raster(ctx, g, tile, v, i, d, pitch=w + 3)
    assert equal(gpu_depth(ctx, g, tile, v, i, d, pitch=w + 3), want["depth"])
    assert equal(gpu_depth(ctx, g, tile, v, i, d, pitch=w + 3, scratch="minimum"), want["depth"])


# ---- 8. the light camera
@pytest.mark.gpu
@pytest.mark.parametrize("mw,mh", [(96, 40), (64, 64)])
def test_light_camera(ctx, mw, mh):
    g, ms = sc.globals_of("default", 70, 45)
    v, i, d = ms.arrays()
    mn, mx = sc.world_box(g, ms)
    light_g, _ = api.sun_fit(sc.world_dir(g, sc.SUN_VIEW).astype(np.float32), mn, mx, mw, mh)
    tile = Tile(0, 0, mw, mh, mw, mh)
    want = gpu_raster(ctx, light_g, tile, v, i, d)
    assert (want["stencil"] > 1).any() and (want["stencil"] == 0).any()
    assert equal(gpu_depth(ctx, light_g, tile, v, i, d, pitch=mw + 16), want["depth"])


# ---- 7. refusals
@pytest.mark.gpu
def test_refusals_enqueue_nothing(ctx):
    W, H = 40, 24
    g, v, i, d = random_scene(W, H, 7, n=32)
    n = int((d["index_count"] // 3).sum())
    tile = Tile(0, 0, W, H, W, H)
    dv, di, dd = ctx.upload(v), ctx.upload(i), ctx.upload(d)
    scratch = ctx.alloc_depth_raster_scratch(W, H, n)
    least = ctx.depth_raster_scratch_bytes(W, H, n, minimum=True)
    t = Target(ctx, tile, W + 3)
    st = ctx.alloc_cull_stats()
    bounds = ctx.upload(np.zeros(len(d) * 6, np.float32))
    keep = []

    def desc(**over):
        f = dict(g=C.addressof(g), tile=C.addressof(tile), vertices=dv.data_ptr(), indices=di.data_ptr(), draws=dd.data_ptr(), depth=t.ptr,
                 scratch=scratch.data_ptr(), scratch_bytes=scratch.numel(), bounds=None, stats=None, n_vertices=len(v), n_indices=len(i),
                 n_draws=len(d), max_triangles=n, pitch=t.pitch, reserved=0)
        f.update(over)
        return DepthRasterDesc(**f)

    def with_tile(*a):
        keep.append(Tile(*a))
        return desc(tile=C.addressof(keep[-1]))

    bad = {
        "null g": desc(g=None), "null tile": desc(tile=None), "null vertices": desc(vertices=None), "null indices": desc(indices=None),
        "null draws": desc(draws=None), "null depth": desc(depth=None), "null scratch": desc(scratch=None),
        "no vertices": desc(n_vertices=0), "no indices": desc(n_indices=0), "no draws": desc(n_draws=0), "no triangles": desc(max_triangles=0),
        "too many draws": desc(n_draws=65536 + 1), "too many triangles": desc(max_triangles=(1 << 22) + 1),
        "empty tile": with_tile(0, 0, 0, H, W, H), "tile outside its frame": with_tile(8, 0, W, H, W, H),
        "frame too large": with_tile(0, 0, W, H, 8192 + 1, H), "empty frame": with_tile(0, 0, W, H, 0, 0),
        "pitch < w": desc(pitch=W - 1),
        "depth misaligned": desc(depth=t.ptr + 2), "vertices misaligned": desc(vertices=dv.data_ptr() + 2),
        "indices misaligned": desc(indices=di.data_ptr() + 1), "draws misaligned": desc(draws=dd.data_ptr() + 2),
        "scratch misaligned": desc(scratch=scratch.data_ptr() + 8, scratch_bytes=scratch.numel() - 8),
        "bounds misaligned": desc(bounds=bounds.data_ptr() + 2), "stats misaligned": desc(bounds=bounds.data_ptr(), stats=st.data_ptr() + 2),
        "stats without bounds": desc(stats=st.data_ptr()),
        "scratch below the minimum": desc(scratch_bytes=least - 1),
        "reserved": desc(reserved=1),
    }
    for what, dsc in bad.items():
        assert ctx.lib.pbr_depth_raster(ctx.h, C.byref(dsc)) == -1, what
        assert ctx.lib.pbr_last_error(ctx.h), what
        assert t.untouched(), what
    assert ctx.lib.pbr_depth_raster(ctx.h, None) == -1 and t.untouched()
    with pytest.raises(PbrError):
        ctx.depth_raster(g, tile, dv, len(v), di, len(i), dd, len(d), n, t.ptr, t.pitch, scratch, stats=st)
    assert t.untouched()
    # the next valid call works: the minimum itself is accepted
    assert ctx.lib.pbr_depth_raster(ctx.h, C.byref(desc(scratch_bytes=least))) == 0
    want = gpu_raster(ctx, g, tile, v, i, d)
    assert equal(t.depth(), want["depth"]) and (want["stencil"] > 0).any()
