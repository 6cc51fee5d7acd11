"""Test images of the anti-aliasing pass, shared by tests/test_fxaa_cpu.py and tests/test_gpu_fxaa.py: uint32 [h, w] RGBA8 arrays
(R in the low byte), every one deterministic.  Alpha varies from pixel to pixel wherever a test could tell."""
import numpy as np

from fxaa_ref import rgba

DARK, BRIGHT = rgba(20, 24, 30, 200), rgba(200, 210, 190, 255)
SLOPES = (1 / 16, 1 / 8, 1 / 5, 1 / 3, 3.0, 5.0, 8.0, 16.0)
OFFSETS = (1 / 8, 1 / 8 + 1 / 3, 1 / 8 + 2 / 3)                 # sub-pixel shifts of the half-plane's edge
COLOUR_PAIRS = (((0, 0, 0), (255, 255, 255)), ((200, 40, 30), (20, 60, 180)), ((96, 128, 64), (250, 235, 120)))


def noise(w, h, seed=0):
    """independent random bytes: nearly every pixel passes the contrast test and every walk ends at once"""
    return np.random.default_rng(seed).integers(0, 2 ** 32, (h, w), dtype=np.uint32)


def blobs(w, h, seed=1):
    """a thresholded sum of a few low-frequency waves: long curved edges between two colours, with a little alpha variation"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    f = np.zeros((h, w))
    for _ in range(5):
        kx, ky, ph = rng.uniform(-0.12, 0.12), rng.uniform(-0.12, 0.12), rng.uniform(0, 6.28)
        f += np.sin(kx * xx + ky * yy + ph)
    img = np.where(f > 0.2, BRIGHT, DARK).astype(np.uint32)
    return img ^ (((xx.astype(np.uint32) * 7 + yy.astype(np.uint32) * 13) & 31) << 24)


def coverage(w, h, slope, sign, offset, through=None, ss=16):
    """the fraction of each pixel on the c1 side of a straight edge.  slope <= 1: the pixels above the line
    y = y0 + offset + sign * slope * (x - x0); slope > 1 (a steep edge): the pixels left of x = x0 + offset + sign * (y - y0) / slope.
    (x0, y0) = `through` in pixel coordinates (pixel (i, j) covers [i, i + 1) x [j, j + 1); default: the image's centre), offset a
    shift across the edge in pixels.  ss x ss samples per pixel; ss = 1 samples the pixel centre."""
    cx, cy = (w / 2, h / 2) if through is None else through
    sub = (np.arange(ss) + 0.5) / ss
    ys = (np.arange(h)[:, None] + sub[None, :]).reshape(-1)
    xs = (np.arange(w)[:, None] + sub[None, :]).reshape(-1)
    yy, xx = np.meshgrid(ys, xs, indexing="ij")
    if slope <= 1:
        inside = yy - (cy + offset) < sign * slope * (xx - cx)
    else:
        inside = xx - (cx + offset) < sign * (yy - cy) / slope
    return inside.reshape(h, ss, w, ss).mean(axis=(1, 3))


def blend(cov, c0, c1):
    """coverage -> RGBA8 image: c0 where cov = 0, c1 where cov = 1, rounded to the nearest byte; alpha 255"""
    c0, c1 = np.asarray(c0, dtype=np.float64), np.asarray(c1, dtype=np.float64)
    b = np.floor(cov[..., None] * c1 + (1 - cov[..., None]) * c0 + 0.5).astype(np.uint32)
    return b[..., 0] | b[..., 1] << 8 | b[..., 2] << 16 | np.uint32(255) << 24


def half_plane(w, h, slope, sign, offset, pair=COLOUR_PAIRS[0], through=None):
    """a hard half-plane edge sampled at the pixel centres"""
    return blend(coverage(w, h, slope, sign, offset, through, ss=1), *pair)


def line(w, h, y):
    """a one-pixel bright horizontal line on dark, from column 3 to the right border"""
    img = np.full((h, w), DARK, dtype=np.uint32)
    img[y, 3:] = BRIGHT
    return img


def checkerboard(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where((xx + yy) & 1, BRIGHT, DARK).astype(np.uint32)


def step(w, h, y0, x_from=0, x_to=None):
    """dark above row y0, bright from it down, between columns x_from and x_to (outside them: dark everywhere)"""
    img = np.full((h, w), DARK, dtype=np.uint32)
    img[y0:, x_from:x_to] = BRIGHT
    return img


def border_edges(w, h):
    """bright first and last rows and columns around a dark field: edges that lie on the frame's border"""
    img = np.full((h, w), DARK, dtype=np.uint32)
    img[0, :] = img[-1, :] = BRIGHT
    img[:, 0] = img[:, -1] = BRIGHT
    return img


def jog(w, h, y0, x0):
    """a horizontal step with one jog: bright from row y0 down left of column x0, from row y0 + 1 down from x0 on"""
    img = np.full((h, w), DARK, dtype=np.uint32)
    img[y0:, :x0] = BRIGHT
    img[y0 + 1:, x0:] = BRIGHT
    return img


def structured(w, h):
    """name -> image: the structured contents at one size (w, h >= 8)"""
    out = {"noise": noise(w, h), "blobs": blobs(w, h), "checkerboard": checkerboard(w, h), "line": line(w, h, h // 2),
           "step": step(w, h, h // 2), "border": border_edges(w, h), "jog": jog(w, h, h // 2, w // 2),
           "half-plane shallow": half_plane(w, h, 1 / 5, 1, 0.31, COLOUR_PAIRS[1]), "half-plane steep": half_plane(w, h, 3.0, -1, 0.0, COLOUR_PAIRS[2])}
    out["vertical step"] = np.ascontiguousarray(step(h, w, w // 2).T)
    return out
