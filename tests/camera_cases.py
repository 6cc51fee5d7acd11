"""Named cameras and camera-dependent scenes for the tests that hold every camera-dependent kernel to its reference under a camera
that pitches and rolls (test_cameras_cpu.py, test_gpu_cameras.py, test_gpu_raster.py, test_gpu_raster_tex.py).

scene.Camera.reference_default has the rotation block diag(-1, 1, -1): its own transpose, middle row and column (0, 1, 0).  A
transposed InvView / View index, or a wrong x or z part of a term that multiplies InvView's middle column, is invisible under it —
and under a yaw-only camera, which leaves InvView[1] = InvView[3] = InvView[5] = InvView[7] = 0.  `default` stays as the control."""
import numpy as np

import common
from direct12pbrrenderer_amd import scene, synth
from direct12pbrrenderer_amd.structs import Tile, cube_mip_offset

PI = float(scene.PI)      # the reference's float32 pi: `default` is scene.Camera.reference_default to the bit
# name: (fov / pi, near, far, position, (roll, yaw, pitch)) — Camera(fov * pi, W, H, near, far); move(position); rotate(roll, yaw, pitch)
CAMERAS = {
    "default": (0.333, 0.1, 1000.0, (0.0, 3.0, 10.0), (0.0, PI, 0.0)),
    "pitch_roll": (0.28, 0.25, 400.0, (1.5, 2.0, 8.0), (0.3, PI + 0.7, -0.4)),
    "roll_only": (0.333, 0.1, 1000.0, (0.0, 3.0, 10.0), (0.9, PI, 0.0)),
    "pitch_only": (0.45, 0.5, 150.0, (-2.0, 5.0, -3.0), (0.0, 0.4, 0.6)),
}
NAMES = tuple(CAMERAS)
NON_DEFAULT = NAMES[1:]

SEED_CAMERA_LIGHTS = 0x5EED0200
LIGHT_BOX = ((-30.0, 30.0), (-20.0, 20.0), (-10.0, 70.0))     # view space: reaches behind the camera and outside every frustum
LIGHT_RADII = (0.5, 1.0, 2.0)


def camera(name, width, height):
    fov, near, far, pos, rot = CAMERAS[name]
    cam = scene.Camera(scene.f32(fov) * scene.PI, width, height, near, far)
    cam.move(pos)
    cam.rotate(*rot)
    return cam


def make_global(name, width, height, sh=None):
    cam = camera(name, width, height)
    return cam, scene.make_global(cam, width, height, sh_pack=sh)


def lights_around(n, cam, seed=SEED_CAMERA_LIGHTS):
    """n lights uniform in LIGHT_BOX of the camera's view space, moved to world space with its world matrix; per light a Radius drawn
    from LIGHT_RADII (its attenuation polynomial is the preset's of that radius) and an Intensity uniform in [1, 10]: the cull's
    Radius * 1.814 * sqrt(Intensity) differs from light to light.  The first k lights of lights_around(n) are lights_around(k)."""
    if n == 0:
        return scene.make_lights(np.zeros((0, 3)), np.zeros((0, 3)), 2.0, 10.0)
    i = np.arange(n, dtype=np.uint64)
    u = [synth._unit(synth.hash_stream(i, seed, k)) for k in range(8)]
    pv = np.stack([lo + (hi - lo) * u[k] for k, (lo, hi) in enumerate(LIGHT_BOX)] + [np.ones(n)], axis=1)
    pw = (cam.world_matrix().astype(np.float64) @ pv.T).T[:, :3]
    lights = scene.make_lights(pw.astype(np.float32), np.stack([u[3], u[4], u[5]], axis=1).astype(np.float32), 2.0, 10.0)
    pick = np.minimum((u[6] * len(LIGHT_RADII)).astype(np.int64), len(LIGHT_RADII) - 1)
    for k, radius in enumerate(LIGHT_RADII):
        r, c0, c1, c2 = scene.attenuation_coefficients(radius)
        for name, val in (("Radius", r), ("C0", c0), ("C1", c1), ("C2", c2)):
            lights[name][pick == k] = np.float32(val)
    lights["Intensity"] = (1.0 + 9.0 * u[7]).astype(np.float32)
    return lights


def view_space(g, positions):
    """world positions -> view space with g.View, float64"""
    view = np.array(g.View[:], dtype=np.float64).reshape(4, 4)
    p = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    return (view @ np.c_[p, np.ones(len(p))].T).T[:, :3]


def world_space(g, positions_view):
    """view-space positions -> world space with g.InvView, float32 records as a light array holds them"""
    inv = np.array(g.InvView[:], dtype=np.float64).reshape(4, 4)
    p = np.asarray(positions_view, dtype=np.float64).reshape(-1, 3)
    return (inv @ np.c_[p, np.ones(len(p))].T).T[:, :3].astype(np.float32)


def shade_scene(name, w, h, n_lights, sh, full=None, x0=0, y0=0, rough_min=0, coverage_mask=True):
    """common.shade_scene under the named camera: the G-buffer's depth plane is made for the camera's Near / Far, the lights are
    lights_around()."""
    full_w, full_h = full if full else (w, h)
    cam, g = make_global(name, full_w, full_h, sh)
    lights = lights_around(n_lights, cam)
    gb = synth.gbuffer_tile(x0, y0, w, h, full_w, full_h, near=float(cam.near), far=float(cam.far), rough_min=rough_min,
                            coverage_mask=coverage_mask)
    return cam, g, lights, gb, Tile(x0, y0, w, h, full_w, full_h)


# ---- the shapes and cases both test files walk
SHADE_SHAPES = ((64, 64, None, 0, 0), (200, 37, (640, 360), 328, 91))     # w, h, full, x0, y0: a frame, a ragged tile of a larger one
SHADE_LIGHTS = (0, 7, 256, 1024)
SHADE_ROUGH = (48, 0)
BOX_FRAMES = ((640, 360), (512, 512), (360, 640))
CULL_FRAME = (640, 360)
CULL_LIGHTS = (300, 1024)
CULL_MARGIN = 1e-4
POSITION_LIGHTS_VIEW = ((0.0, 0.0, 8.0), (-6.0, 3.0, 20.0), (5.0, -2.0, 4.0), (10.0, 5.0, 40.0))
POSITION_ROUGH_MIN = 128
POSITION_C2 = 0.01


def position_light(g, p_view, c2):
    """one white light of intensity 10 at view-space p_view with the attenuation polynomial 1 + c2 d^2"""
    l = scene.make_lights(world_space(g, [p_view]), [[1.0, 1.0, 1.0]], 2.0, 10.0)
    l["C0"], l["C1"], l["C2"] = np.float32(1.0), np.float32(0.0), np.float32(c2)
    return l


def cluster_table(template, every):
    """a cluster table with the boxes of `template` whose every cluster lists light 0 (every) or nothing"""
    cl = template.copy()
    cl["NumLights"] = 1 if every else 0
    cl["LightIndex"] = 0
    return cl


def position_ratio(i0, ia, ib):
    """(selected pixels, measured ratio (IA - I0) / (IB - I0) in the channel where IA - I0 is largest, allowed relative error), the
    bound from 1e-4 * scale of L-inf on each of the four values entering the ratio: 4e-4 * scale / (IB - I0) <= 0.05 where selected"""
    i0, ia, ib = (np.asarray(a, dtype=np.float64)[..., :3] for a in (i0, ia, ib))
    scale = float(np.abs(ia).max())
    da, db = ia - i0, ib - i0
    ch = da.argmax(axis=-1)[..., None]
    da, db = np.take_along_axis(da, ch, -1)[..., 0], np.take_along_axis(db, ch, -1)[..., 0]
    sel = db >= 0.008 * scale
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(sel, da / db, 0.0)
        tol = np.where(sel, 4e-4 * scale / db, 0.0)
    return sel, ratio, tol


# ---- the sky of the skybox test: 64^2 faces of 8 x 8 blocks of 8 x 8 texels, one colour per block, exact in half
SKY_SIZE, SKY_BLOCK, SKY_MIPS = 64, 8, 7


def block_colours():
    """[6, 8, 8, 3]: k / 256 with k < 2048 — exact in half, distinct per block (the red channel alone tells the 384 blocks apart)"""
    ident = np.arange(6 * 8 * 8).reshape(6, 8, 8)
    return np.stack([(ident + 1) / 256.0, ((ident * 7) % 384 + 1) / 256.0, ((ident * 13) % 384 + 1) / 256.0], axis=-1)


def block_sky():
    """the cube in the pbr_cube_f32 layout, mip 0 filled (the oracle's box mips make the rest)"""
    out = np.zeros(4 * cube_mip_offset(SKY_SIZE, SKY_MIPS), dtype=np.float32)
    m0 = out[: 4 * 6 * SKY_SIZE * SKY_SIZE].reshape(6, SKY_SIZE, SKY_SIZE, 4)
    m0[..., :3] = np.repeat(np.repeat(block_colours(), SKY_BLOCK, axis=1), SKY_BLOCK, axis=2).astype(np.float32)
    m0[..., 3] = 1.0
    return out


# ---- the oracle's side of a case, computed the same way by the CPU file (which asserts the preconditions) and the GPU file
def oracle_shade(orc, ibl, name, shape, n_lights, rough_min):
    """the named camera's scene of `shape` with its oracle cluster table, fp16 and fp32 oracle images and the f64 truth"""
    sky, env, lut, sh = ibl
    w, h, full, x0, y0 = shape
    cam, g, lights, gb, tile = shade_scene(name, w, h, n_lights, sh, full=full, x0=x0, y0=y0, rough_min=rough_min)
    cl = orc.cluster_build(g)
    orc.cluster_cull(g, lights, cl)
    want, want_f32 = orc.deferred_shade(g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights, want_f32=True)
    truth = orc.deferred_shade_f64(g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights)
    return dict(g=g, lights=lights, gb=gb, tile=tile, cl=cl, want=want, want_f32=want_f32, truth=truth, rough=gb["C"] & 255)


def position_scene(name, shape, sh):
    """the world-position check's scene: rough_min 128 keeps the BRDF tame, every pixel shaded"""
    w, h, full, x0, y0 = shape
    return shade_scene(name, w, h, 0, sh, full=full, x0=x0, y0=y0, rough_min=POSITION_ROUGH_MIN, coverage_mask=False)


# the folded / tabled shade: the shapes of test_gpu_shade_tables.py (a 600 x 40 tile of a 4K frame, a 256 x 64 frame), 300 lights
FOLD_TILE = (600, 40, (3840, 2160), 1300, 1000)
FOLD_SMALL = (256, 64, None, 0, 0)
FOLD_LIGHTS = 300
FOLD_TILE_ROUGH_MIN = 48      # the tile's image is also held to the oracle on the fp16 target: no GGX peak beyond the half range

SKY_FRAME = (640, 360)        # magnified: every pixel samples LOD 0
# A bilinear tap at LOD 0 reaches half a texel, the sampler's fixed-point snap 1 / 256 more: a pixel whose face coordinate is a whole
# texel inside its block reads that block alone.  (Two texels would leave three quarters of the frame unchecked.)
SKY_MARGIN = 1.0


def sky_expectation(camera_ref, g, tile):
    """(block colour [h, w, 3] half of the block every pixel's view ray lands in, mask of the pixels at least SKY_MARGIN texels inside
    their block), from camera_ref.ray_dirs()"""
    face, x, y = camera_ref.cube_face_coords(camera_ref.ray_dirs(g, tile), SKY_SIZE)
    fx, fy = x % SKY_BLOCK, y % SKY_BLOCK
    inside = (fx >= SKY_MARGIN) & (fx <= SKY_BLOCK - SKY_MARGIN) & (fy >= SKY_MARGIN) & (fy <= SKY_BLOCK - SKY_MARGIN)
    bx, by = (np.clip(c // SKY_BLOCK, 0, SKY_SIZE // SKY_BLOCK - 1).astype(np.int64) for c in (x, y))
    return block_colours().astype(np.float16)[face, by, bx], inside
