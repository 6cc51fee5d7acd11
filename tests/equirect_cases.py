"""The cases and the bound of the pbr_equirect_to_cube tests, shared by test_equirect_cpu.py and test_gpu_equirect.py.

The bound is derived, not measured.  The coordinate chain is one division, atan2f (OpenCL allows it 6 ulp), a sqrt and five more
roundings at magnitudes <= max(pw, ph): delta = 16 * 2^-24 * max(pw, ph) texels of coordinate error.  Bilinear interpolation is
continuous and piecewise linear with slope <= L per texel in each axis, so a coordinate error of delta in s and in t moves a sample by
at most 2 delta L; the three lerps round five times per sample (<= 8 * 2^-24 M with the differences' own roundings) and the sum of
samples^2 samples another samples^2 times:
    |texel - float64 restatement| <= 2 delta L + (samples^2 + 8) 2^-24 M          per channel, no texel set aside
with L the largest difference between horizontally (wrapping) or vertically adjacent panorama texels and M the largest |texel|."""
import functools

import numpy as np

import equirect_ref as ref

# (pw, ph, size, samples)
CASES = [
    (8, 4, 4, 1),             # the smallest plain shape
    (7, 5, 3, 1),             # everything odd: a sample exactly on +-Y (the lambda = 0 rule) and exactly on the seam column
    (16, 8, 5, 2),            # odd size with sub-samples
    (64, 32, 12, 4),          # samples = 4
    (128, 64, 40, 1),         # several blocks per face, a ragged last tile
    (2048, 1024, 8, 8),       # strong minification, 64 samples per texel
    (16384, 8, 4, 2),         # the largest coordinates (one noise row repeated)
]
DEGENERATE = [(1, 1, 2, 1), (2, 1, 1, 1)]      # the wraps of a one- and a two-column panorama
ALL_CASES = CASES + DEGENERATE
RGBE_CASES = [(7, 5, 3, 1), (64, 32, 12, 4), (128, 64, 40, 1)]


def case_id(c):
    return "%dx%d-%d-s%d" % c


@functools.lru_cache(maxsize=None)
def panorama(pw, ph):
    """seeded uniform noise in [0, 1), float32 [ph, pw, 4] (alpha 1); the 16384-wide case is one noise row repeated"""
    rng = np.random.default_rng(1000003 * pw + ph)
    if pw == 16384:
        rgb = np.repeat(rng.random((1, pw, 3), dtype=np.float32), ph, axis=0)
    else:
        rgb = rng.random((ph, pw, 3), dtype=np.float32)
    p = np.ones((ph, pw, 4), dtype=np.float32)
    p[..., :3] = rgb
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def truth(pw, ph, size, samples):
    """the float64 restatement of a case, computed once per process and left unchanged"""
    t = ref.equirect_to_cube(panorama(pw, ph), size, samples, np.float64)
    t.setflags(write=False)
    return t


def bound(pano, samples):
    """2 delta L + (samples^2 + 8) 2^-24 M of the module docstring"""
    rgb = np.asarray(pano)[..., :3].astype(np.float64)
    ph, pw = rgb.shape[:2]
    L = float(np.abs(rgb - np.roll(rgb, -1, axis=1)).max())
    if ph > 1:
        L = max(L, float(np.abs(rgb[1:] - rgb[:-1]).max()))
    M = float(np.abs(rgb).max())
    delta = 16.0 * 2.0 ** -24 * max(pw, ph)
    return 2.0 * delta * L + (samples * samples + 8) * 2.0 ** -24 * M


@functools.lru_cache(maxsize=None)
def rgbe_panorama(pw, ph):
    """seeded RGBE bytes [ph, pw, 4] with moderate exponents, plus texels of exponent 0 (decode to 0 whatever the mantissas) and of
    exponent 255 (the largest scale, 2^119: finite)"""
    rng = np.random.default_rng(77 * pw + ph)
    b = rng.integers(0, 256, size=(ph, pw, 4), dtype=np.uint8)
    b[..., 3] = rng.integers(120, 140, size=(ph, pw), dtype=np.uint8)
    flat = b.reshape(-1, 4)
    flat[1, 3] = 0
    flat[len(flat) // 2, 3] = 0
    flat[3, 3] = 255
    flat[-2, 3] = 255
    flat[5, 3] = 1             # the smallest scale, 2^-135: subnormal products
    b.setflags(write=False)
    return b


# ---- the convention, held to analytic truth the restatement did not write ---------------------------------------------------------
ANALYTIC_C = np.array([0.25, 0.125, -0.2])
ANALYTIC_PW, ANALYTIC_PH, ANALYTIC_SIZE = 64, 32, 8
# the latitude clamp at the poles + the interpolation error of a function whose second derivative along a unit direction is <= |c|_1
ANALYTIC_BOUND = (np.pi / (2 * ANALYTIC_PH) + ((2 * np.pi / ANALYTIC_PW) ** 2 + (np.pi / ANALYTIC_PH) ** 2) / 8) * np.abs(ANALYTIC_C).sum()


def analytic_f(d):
    """f(d) = 0.6 + c . d of unit directions d [..., 3]"""
    return 0.6 + d @ ANALYTIC_C


@functools.lru_cache(maxsize=None)
def analytic_panorama():
    """f at the texel-centre directions of a 64 x 32 panorama: the centre column looks along +Z, columns advance towards +X, row 0 is
    +Y — written from the convention's words, not from the rule's formulas.  float32 [ph, pw, 4], the three channels equal."""
    pw, ph = ANALYTIC_PW, ANALYTIC_PH
    lon = ((np.arange(pw) + 0.5) / pw - 0.5) * 2.0 * np.pi          # 0 at the centre, growing to the right
    lat = (np.arange(ph) + 0.5) / ph * np.pi                         # the polar angle from +Y, 0 at the top
    sin_t, cos_t = np.sin(lat)[:, None], np.cos(lat)[:, None]
    d = np.stack([sin_t * np.sin(lon)[None, :], cos_t * np.ones((1, pw)), sin_t * np.cos(lon)[None, :]], axis=-1)
    p = np.ones((ph, pw, 4), dtype=np.float32)
    p[..., :3] = analytic_f(d)[..., None]
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def analytic_expected():
    """f at the centre direction of every texel of a size-8 cube, [6, 8, 8]: the faces' directions as D3D defines a cube map
    (+X: (1, -v, -u), -X: (-1, -v, u), +Y: (u, 1, v), -Y: (u, -1, -v), +Z: (u, -v, 1), -Z: (-u, -v, -1)), normalised"""
    n = ANALYTIC_SIZE
    c = (np.arange(n) + 0.5) / n * 2.0 - 1.0
    u, v = np.meshgrid(c, c)          # u along x, v along y
    one = np.ones_like(u)
    dirs = [(one, -v, -u), (-one, -v, u), (u, one, v), (u, -one, -v), (u, -v, one), (-u, -v, -one)]
    out = np.zeros((6, n, n))
    for f, (x, y, z) in enumerate(dirs):
        d = np.stack([x, y, z], axis=-1)
        out[f] = analytic_f(d / np.linalg.norm(d, axis=-1, keepdims=True))
    out.setflags(write=False)
    return out


# ---- the two default rules: (pw, size the import picks); (pw, size, samples it picks) ----------------------------------------------
DEFAULT_SIZE_TABLE = [(1, 4), (7, 4), (16, 4), (31, 4), (32, 8), (63, 8), (64, 16), (1000, 128), (1024, 256), (2048, 512), (4096, 1024),
                      (8192, 2048), (16384, 4096), (32768, 8192), (65536, 8192), (4000000000, 8192)]
DEFAULT_SAMPLES_TABLE = [(64, 16, 1), (65, 16, 2), (128, 16, 2), (129, 16, 4), (256, 16, 4), (257, 16, 8), (512, 16, 8), (100000, 16, 8),
                         (1, 4, 1), (16, 4, 1), (17, 4, 2), (1000, 128, 2), (8192, 2048, 1), (16384, 8192, 1), (4000000000, 8192, 8)]
