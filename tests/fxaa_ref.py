"""The anti-aliasing rule of pbr_fxaa (include/pbr_hip.h, "Anti-aliasing"), restated twice: pixel() is the rule for one pixel in plain
Python integers, fxaa() the same rule on whole planes in numpy.  The two share no code beyond the constants; tests/test_fxaa_cpu.py
holds them equal, and every GPU comparison (tests/test_gpu_fxaa.py) is exact equality with fxaa().

An image is a uint32 [h, w] array of RGBA8 pixels, R in the low byte (what DeferredFrame.ldr_numpy() returns).  The rule is integer
arithmetic throughout: there is no tolerance anywhere.

fxaa(..., defect=NAME) runs the rule with one deliberate mistake (DEFECTS): the CPU tests show that each one trips an assertion."""
import numpy as np

OFFSETS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24)
REACH = OFFSETS[-1] + 1          # the farthest pixel the rule reads from M, along either axis
EDGE_MIN = 4080                  # 16 grey levels: 16 * (77 + 150 + 29)
DEFECTS = ("luma", "hv", "good", "dirs", "wrap", "round", "kn_only", "tie")


# ---- the scalar form ------------------------------------------------------------------------------------------------------------
def pixel(img, x, y):
    """-> (the filtered pixel, None for a pixel that fails the contrast test or a dict of the rule's intermediate values)"""
    h, w = img.shape

    def px(xx, yy):
        return int(img[min(max(yy, 0), h - 1), min(max(xx, 0), w - 1)])

    def lum(xx, yy):
        p = px(xx, yy)
        return 77 * (p & 255) + 150 * ((p >> 8) & 255) + 29 * ((p >> 16) & 255)

    m, n, s, we, e = lum(x, y), lum(x, y - 1), lum(x, y + 1), lum(x - 1, y), lum(x + 1, y)
    hi, lo = max(m, n, s, we, e), min(m, n, s, we, e)
    rng = hi - lo
    if rng < max(EDGE_MIN, hi >> 3):
        return px(x, y), None
    nw, ne, sw, se = lum(x - 1, y - 1), lum(x + 1, y - 1), lum(x - 1, y + 1), lum(x + 1, y + 1)
    eh = abs(nw + sw - 2 * we) + 2 * abs(n + s - 2 * m) + abs(ne + se - 2 * e)
    ev = abs(nw + ne - 2 * n) + 2 * abs(we + e - 2 * m) + abs(sw + se - 2 * s)
    horz = eh >= ev
    a, b = (n, s) if horz else (we, e)
    side_b = not abs(a - m) >= abs(b - m)
    g = abs(b - m) if side_b else abs(a - m)
    step = 1 if side_b else -1
    ax, ay, cx, cy = (1, 0, 0, step) if horz else (0, 1, step, 0)
    nb = lum(x + cx, y + cy)
    p2, m_lt = m + nb, m < nb

    def walk(d):
        for k in OFFSETS:
            err = lum(x + d * k * ax, y + d * k * ay) + lum(x + d * k * ax + cx, y + d * k * ay + cy) - p2
            if 2 * abs(err) >= g:
                break
        return k, err

    (kn, en), (kp, ep) = walk(-1), walk(+1)
    if kn < kp:
        dst, good = kn, (en < 0) != m_lt
    else:
        dst, good = kp, (ep < 0) != m_lt
    off8 = 128 - (256 * dst) // (kn + kp) if good else 0
    t = min(256, (256 * abs(2 * (n + s + we + e) + nw + ne + sw + se - 12 * m)) // (12 * rng))
    sm = (t * t * (768 - 2 * t)) >> 16
    sub8 = (3 * sm * sm) >> 10
    f8 = max(off8, sub8)
    pm, pn = px(x, y), px(x + cx, y + cy)
    out = pm & 0xFF000000
    for sh in (0, 8, 16):
        out |= ((((pm >> sh) & 255) * (256 - f8) + ((pn >> sh) & 255) * f8 + 128) >> 8) << sh
    return out, dict(horz=horz, side_b=side_b, kn=kn, kp=kp, off8=off8, sub8=sub8, f8=f8, nb=(x + cx, y + cy))


def fxaa_scalar(img):
    img = np.ascontiguousarray(img, dtype=np.uint32)
    out = np.empty_like(img)
    for y in range(img.shape[0]):
        for x in range(img.shape[1]):
            out[y, x] = pixel(img, x, y)[0]
    return out


# ---- the vectorised form ----------------------------------------------------------------------------------------------------------
def luma(img, weights=(77, 150, 29)):
    p = np.asarray(img, dtype=np.uint32).astype(np.int64)
    return weights[0] * (p & 255) + weights[1] * ((p >> 8) & 255) + weights[2] * ((p >> 16) & 255)


def fxaa(img, defect=None, details=False):
    """-> the filtered image; with details (image, dict of planes: edge, horz, side_b, kn, kp, off8, sub8, f8; zero off the edge pixels)"""
    assert defect is None or defect in DEFECTS
    img = np.ascontiguousarray(img, dtype=np.uint32)
    h, w = img.shape
    lum = luma(img, (150, 77, 29) if defect == "luma" else (77, 150, 29))
    yy, xx = np.mgrid[0:h, 0:w]

    def at(plane, x, y):
        if defect == "wrap":
            return plane[y % h, x % w]
        return plane[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]

    t = {name: at(lum, xx + dx, yy + dy) for name, dx, dy in
         (("m", 0, 0), ("n", 0, -1), ("s", 0, 1), ("w", -1, 0), ("e", 1, 0), ("nw", -1, -1), ("ne", 1, -1), ("sw", -1, 1), ("se", 1, 1))}
    five = np.stack([t[k] for k in "mnswe"])
    hi, lo = five.max(axis=0), five.min(axis=0)
    rng = hi - lo
    edge = rng >= np.maximum(EDGE_MIN, hi >> 3)
    eh = np.abs(t["nw"] + t["sw"] - 2 * t["w"]) + 2 * np.abs(t["n"] + t["s"] - 2 * t["m"]) + np.abs(t["ne"] + t["se"] - 2 * t["e"])
    ev = np.abs(t["nw"] + t["ne"] - 2 * t["n"]) + 2 * np.abs(t["w"] + t["e"] - 2 * t["m"]) + np.abs(t["sw"] + t["se"] - 2 * t["s"])
    horz = eh < ev if defect == "hv" else eh >= ev
    a, b = np.where(horz, t["n"], t["w"]), np.where(horz, t["s"], t["e"])
    da, db = np.abs(a - t["m"]), np.abs(b - t["m"])
    side_b = ~(da > db) if defect == "tie" else ~(da >= db)
    g = np.where(side_b, db, da)
    step = np.where(side_b, 1, -1)
    ax, ay = horz.astype(np.int64), (~horz).astype(np.int64)
    cx, cy = np.where(horz, 0, step), np.where(horz, step, 0)
    nb = at(lum, xx + cx, yy + cy)
    p2, m_lt = t["m"] + nb, t["m"] < nb

    def walk(d):
        k_end = np.full((h, w), OFFSETS[-1], dtype=np.int64)
        e_end = np.zeros((h, w), dtype=np.int64)
        open_ = edge.copy()
        for k in OFFSETS:
            mx, my = xx + d * k * ax, yy + d * k * ay
            err = at(lum, mx, my) + at(lum, mx + cx, my + cy) - p2
            k_end[open_], e_end[open_] = k, err[open_]
            open_ &= 2 * np.abs(err) < g
        return k_end, e_end

    (kn, en), (kp, ep) = (walk(+1), walk(-1)) if defect == "dirs" else (walk(-1), walk(+1))
    first = np.ones_like(edge) if defect == "kn_only" else kn < kp
    dst = np.where(first, kn, kp)
    good = (np.where(first, en, ep) < 0) != m_lt
    if defect == "good":
        good = np.ones_like(edge)
    off8 = np.where(good, 128 - (256 * dst) // (kn + kp), 0)
    amount = np.abs(2 * (t["n"] + t["s"] + t["w"] + t["e"]) + t["nw"] + t["ne"] + t["sw"] + t["se"] - 12 * t["m"])
    tt = np.minimum(256, (256 * amount) // np.where(edge, 12 * rng, 1))
    sm = (tt * tt * (768 - 2 * tt)) >> 16
    sub8 = (3 * sm * sm) >> 10
    f8 = np.where(edge, np.maximum(off8, sub8), 0)
    pm, pn = img.astype(np.int64), at(img, xx + cx, yy + cy).astype(np.int64)
    out = pm & 0xFF000000
    for sh in (0, 8, 16):
        out |= ((((pm >> sh) & 255) * (256 - f8) + ((pn >> sh) & 255) * f8 + (0 if defect == "round" else 128)) >> 8) << sh
    out = out.astype(np.uint32)
    if not details:
        return out
    z = lambda p: np.where(edge, p, 0)
    return out, dict(edge=edge, horz=z(horz), side_b=z(side_b), kn=z(kn), kp=z(kp), off8=z(off8), sub8=z(sub8), f8=f8)


def edge_mask(img):
    """the pixels that pass the contrast test"""
    return fxaa(img, details=True)[1]["edge"]


def rgba(r, g, b, a=255):
    return np.uint32(int(r) | int(g) << 8 | int(b) << 16 | int(a) << 24)


def channels(img):
    """uint32 [h, w] -> int64 [h, w, 4]"""
    return (np.asarray(img, dtype=np.uint32)[..., None].astype(np.int64) >> np.array([0, 8, 16, 24])) & 255
