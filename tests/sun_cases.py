"""The scenes and cases of the sun-light tests (test_sun_cpu.py, test_gpu_sun.py, test_gpu_sun_frame.py): a plate and four strips
hover one unit over a ground quad, all placed in the VIEW space of a named camera (camera_cases.py) so that every camera sees the
same picture; the sun is tilted 30 degrees from the view's up axis.  Camera G-buffer and shadow map of a case come from
tests/raster_ref.py, once per process; the truth (tests/sun_truth.py) is computed once per case and shared.

View space: x right, y up, z into the scene.  Ground: y = -1.5, x in [-4, 4], z in [3, 11].  Casters at y = -0.5 (gap 1): the plate
x in [-3.5, -0.3], z in [4.6, 8.4] (wide enough for a fully shadowed core under the 16 x 16 map's 4-texel pcf footprint), the strips 0.4
wide and 3.5 long (perimeter for the penumbra share).  The shadow of a caster point lies tan(30 deg) = 0.577 from under it."""
import functools
import math

import numpy as np

import camera_cases
import raster_ref
import sun_truth as st
from direct12pbrrenderer_amd import api, scene
from direct12pbrrenderer_amd.structs import Tile

GROUND_Y, CASTER_Y = -1.5, -0.5
GROUND = (-4.0, 4.0, 3.0, 11.0)                      # x0, x1, z0, z1
PLATE = (-3.5, -0.3, 4.6, 8.4)
STRIPS = [(c - 0.2, c + 0.2, 4.5, 8.0) for c in (0.8, 1.6, 2.4, 3.2)]
CASTERS = [PLATE] + STRIPS
TILT, AZIMUTH = math.radians(30.0), math.radians(40.0)
SUN_VIEW = np.array([math.sin(TILT) * math.cos(AZIMUTH), math.cos(TILT), math.sin(TILT) * math.sin(AZIMUTH)])
LUMINANCE = (100.0, 90.0, 70.0)                      # not grey: a permuted channel shows
PLATE_BOX_VIEW = ((-3.9, GROUND_Y, 4.3), (-0.8, CASTER_Y, 8.0))      # the 16 x 16 map is fitted inside the plate's shadow and its rim


def _rect_model(g, rect, y):
    """(mesh, model): a rect = (x0, x1, z0, z1) of the view-space plane y, facing +y, through quad_grid (which faces -z of its plane)"""
    x0, x1, z0, z1 = rect
    to_view = np.array([[1, 0, 0, 0.5 * (x0 + x1)], [0, 0, -1, y], [0, 1, 0, 0.5 * (z0 + z1)], [0, 0, 0, 1]], dtype=np.float64)
    inv_view = np.array(g.InvView[:], dtype=np.float64).reshape(4, 4)
    return (x1 - x0, z1 - z0), (inv_view @ to_view).astype(np.float32)


def mesh_scene(g):
    ms = scene.MeshScene()
    size, model = _rect_model(g, GROUND, GROUND_Y)
    ms.add(scene.quad_grid(4, 4, size=size), model, albedo=(0.8, 0.7, 0.6), roughness=0.6, metallic=0.1)
    for k, rect in enumerate(CASTERS):
        size, model = _rect_model(g, rect, CASTER_Y)
        ms.add(scene.quad_grid(1, 1, size=size), model, albedo=(0.3, 0.5, 0.9), roughness=0.3, metallic=0.7)
    return ms


def world_dir(g, d_view):
    inv_view = np.array(g.InvView[:], dtype=np.float64).reshape(4, 4)[:3, :3]
    d = inv_view @ np.asarray(d_view, dtype=np.float64)
    return d / np.linalg.norm(d)


def world_box(g, ms=None, view_box=None):
    """(min, max) float32 world box: the union of the draws' world boxes (MeshScene.bounds through each Model), or the world box of a
    view-space box's eight corners"""
    if view_box is not None:
        inv_view = np.array(g.InvView[:], dtype=np.float64).reshape(4, 4)
        c = np.array([[view_box[i][0], view_box[j][1], view_box[k][2], 1.0] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
        w = (inv_view @ c.T).T[:, :3]
        return np.floor(w.min(axis=0) * 64) / 64, np.ceil(w.max(axis=0) * 64) / 64
    return scene.world_box(ms.arrays()[2], ms.bounds())


class Case:
    def __init__(self, name, camera, w, h, pitch, map_w, map_h, map_pitch, pcf, shadows=True, fit="union", bias=None):
        self.name, self.camera, self.w, self.h, self.pitch = name, camera, w, h, pitch
        self.map_w, self.map_h, self.map_pitch, self.pcf, self.shadows, self.fit, self.bias = map_w, map_h, map_pitch, pcf, shadows, fit, bias

    def __repr__(self):
        return self.name


# camera targets 70 x 45 at pitch 77 and 256 x 144; maps 16 x 16 (fitted around the plate: most of the ground's footprints leave it),
# 64 x 64 at pitch 80 and 96 x 40; both cameras, both filters, with a map and without.  bias None: acne_free_bias().  The 16 x 16 pcf-3
# case has no bias that is both free of acne and leaves a fully shadowed core (its 4-texel footprint is 1.2 units wide): it takes a small
# one and keeps the acne around the core, which the truth has as well.
CASES = [
    Case("70x45-default-m64-pcf3", "default", 70, 45, 77, 64, 64, 80, 3),
    Case("70x45-pitch_roll-m64-pcf1", "pitch_roll", 70, 45, 77, 64, 64, 80, 1),
    Case("256x144-default-m96x40-pcf3", "default", 256, 144, 256, 96, 40, 96, 3),
    Case("256x144-pitch_roll-m96x40-pcf1", "pitch_roll", 256, 144, 256, 96, 40, 96, 1),
    Case("256x144-default-m16-pcf3", "default", 256, 144, 256, 16, 16, 16, 3, fit="plate", bias=(0.03, 0.0)),
    Case("70x45-pitch_roll-m16-pcf1", "pitch_roll", 70, 45, 77, 16, 16, 16, 1, fit="plate"),
    Case("256x144-default-noshadow", "default", 256, 144, 256, 0, 0, 0, 3, shadows=False),
    Case("70x45-pitch_roll-noshadow", "pitch_roll", 70, 45, 77, 0, 0, 0, 1, shadows=False),
]
BY_NAME = {c.name: c for c in CASES}


def acne_free_bias(ext, map_w, map_h, pcf):
    """(bias_const, 0): the ground is a plane tilted by TILT against the light, so its light depth changes by tan(TILT) per unit of
    light-space x / y; a tap up to r texels from the receiver (r = 1 for the bilinear footprint, 2 for pcf 3) stores a depth up to
    r * (texel diagonal) * tan(TILT) nearer.  1.25 x that, in clip depth units: no acne, and well below the casters' gap of
    cos(TILT) = 0.87 units of depth (peter-panning under a tenth of the shadow's offset at the 64 and 96 maps)."""
    l, r, b, t, n, f = ext
    diag = math.hypot((r - l) / map_w, (t - b) / map_h)
    reach = 1.0 if pcf == 1 else 2.0
    return (1.25 * reach * diag * math.tan(TILT) / (f - n), 0.0)


@functools.lru_cache(maxsize=None)
def globals_of(camera, w, h):
    cam = camera_cases.camera(camera, w, h)
    g = scene.make_global(cam, w, h)
    ms = mesh_scene(g)
    return g, ms


_GB = {}


def camera_gbuffer(case, orc):
    """the camera's five G-buffer planes of the case's scene ([h, w] numpy), from raster_ref, once per (camera, size)"""
    key = (case.camera, case.w, case.h)
    if key not in _GB:
        g, ms = globals_of(*key)
        v, i, d = ms.arrays()
        _GB[key] = raster_ref.raster(g, Tile(0, 0, case.w, case.h, case.w, case.h), v, i, d, orc)
    return _GB[key]


_BUILT = {}


def build(case, orc):
    """Everything of a case, once: dict g, ms, tile, gb (numpy planes), sun (sun_truth dict), sun_dir, light_g, lvp, ext, depth_map
    ([map_h, map_w] float32 or None), light planes (raster_ref's five planes under the light), cam (sun_truth.camera_of), truth,
    restated, details."""
    if case.name in _BUILT:
        return _BUILT[case.name]
    g, ms = globals_of(case.camera, case.w, case.h)
    tile = Tile(0, 0, case.w, case.h, case.w, case.h)
    gb = camera_gbuffer(case, orc)
    sun_dir = world_dir(g, SUN_VIEW)
    out = {"g": g, "ms": ms, "tile": tile, "gb": gb, "sun_dir": sun_dir, "cam": st.camera_of(g), "depth_map": None, "light_g": None,
           "lvp": None, "light": None}
    if case.shadows:
        mn, mx = world_box(g, ms) if case.fit == "union" else world_box(g, view_box=PLATE_BOX_VIEW)
        light_g, lvp = api.sun_fit(sun_dir.astype(np.float32), mn, mx, case.map_w, case.map_h)
        ext = st.sun_fit(sun_dir.astype(np.float32), mn, mx, case.map_w, case.map_h)[4]
        v, i, d = ms.arrays()
        light = raster_ref.raster(light_g, Tile(0, 0, case.map_w, case.map_h, case.map_w, case.map_h), v, i, d, orc)
        bias = case.bias if case.bias is not None else acne_free_bias(ext, case.map_w, case.map_h, case.pcf)
        out.update(light_g=light_g, lvp=lvp, ext=ext, light=light, depth_map=light["depth"], box=(mn, mx))
        out["sun"] = st.make_sun(sun_dir, LUMINANCE, np.array(lvp, dtype=np.float32).reshape(4, 4), bias, case.pcf)
    else:
        out["sun"] = st.make_sun(sun_dir, LUMINANCE, None, (0.0, 0.0), case.pcf)
    details = {}
    out["truth"] = st.truth(out["cam"], tile, gb, out["sun"], out["depth_map"])
    out["restated"] = st.restate(out["cam"], tile, gb, out["sun"], out["depth_map"], details=details)
    out["details"] = details
    _BUILT[case.name] = out
    return out


def api_sun(b):
    """structs.Sun of a built case"""
    s = b["sun"]
    return api.make_sun(s["Direction"], s["Luminance"], s["M"].reshape(16), (float(s["bias_const"]), float(s["bias_slope"])), s["pcf"])


def shadow_polygons_view():
    """the casters' shadows on the ground as view-space (x, z) rectangles' corner lists: a caster point p casts to p - SUN_VIEW * s with
    s = (CASTER_Y - GROUND_Y) / SUN_VIEW.y"""
    s = (CASTER_Y - GROUND_Y) / SUN_VIEW[1]
    off = (-SUN_VIEW[0] * s, -SUN_VIEW[2] * s)
    return [[(x + off[0], z + off[1]) for (x, z) in ((x0, z0), (x1, z0), (x1, z1), (x0, z1))] for (x0, x1, z0, z1) in CASTERS]


def ground_shadow_distance(b):
    """Per pixel of the case's frame: (is_ground, signed distance in view-space units from the pixel's ground point to the boundary of
    the union of the analytic shadows, negative inside a shadow).  The shadows are axis-aligned rectangles in the ground plane."""
    tr = b["truth"]
    view = np.array(b["g"].View[:], dtype=np.float64).reshape(4, 4)
    pv = tr["position"] @ view[:3, :3].T + view[:3, 3]
    is_ground = tr["on"] & (np.abs(pv[..., 1] - GROUND_Y) < 0.05)
    dist = np.full(pv.shape[:2], np.inf)
    for poly in shadow_polygons_view():
        xs, zs = [p[0] for p in poly], [p[1] for p in poly]
        x0, x1, z0, z1 = min(xs), max(xs), min(zs), max(zs)
        dx = np.maximum(x0 - pv[..., 0], pv[..., 0] - x1)
        dz = np.maximum(z0 - pv[..., 2], pv[..., 2] - z1)
        outside = np.hypot(np.maximum(dx, 0.0), np.maximum(dz, 0.0))
        d = np.where((dx <= 0) & (dz <= 0), np.maximum(dx, dz), outside)
        dist = np.minimum(dist, d)
    return is_ground, dist, pv


def tie_case(b):
    """A 1 x 1 map that stores exactly the zr of one lit pixel of a built case (the one nearest the middle of the light's box, where the
    single texel carries nearly all of the bilinear weight): dict pixel (y, x), sun (pcf 1), depth_map [1, 1] and unshadowed, the
    pixel's float32 probe value without a map."""
    sun = dict(b["sun"], pcf=1)
    details = {}
    st.restate(b["cam"], b["tile"], b["gb"], sun, np.ones((1, 1), np.float32), details=details)
    q = b["truth"]["q"]
    cost = np.where(details["lit"], np.abs(q[..., 0]) + np.abs(q[..., 1]), np.inf)
    y, x = np.unravel_index(int(np.argmin(cost)), cost.shape)
    assert cost[y, x] < 0.2
    plain = st.restate(b["cam"], b["tile"], b["gb"], sun, None)
    return {"pixel": (int(y), int(x)), "sun": sun, "depth_map": np.full((1, 1), details["zr"][y, x], np.float32), "unshadowed": plain[y, x].copy()}


def assert_tie_lit(probe_of, tie):
    """probe_of(sun, depth_map) -> float32 probe image [h, w, 4]"""
    y, x = tie["pixel"]
    got = np.asarray(probe_of(tie["sun"], tie["depth_map"]))[y, x]
    assert tie["unshadowed"][:3].max() > 0
    assert np.array_equal(got, tie["unshadowed"]), f"a tie is not lit: pixel ({x}, {y}) holds {got}, unshadowed {tie['unshadowed']}"
