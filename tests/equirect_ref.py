"""numpy restatement of the pbr_equirect_to_cube rule (include/pbr_hip.h, "Equirectangular panoramas"), a function of a dtype: float64
is the truth the kernel is held to within the derived bound of tests/equirect_cases.py, float32 is the rule at the kernel's own
precision and shows that bound to be attainable.  Written from the header's text, step by step; shares nothing with the kernel."""
import numpy as np


def cube_dir_raw(f, a, b):
    """step 2: the cube's face mapping, not normalised (a along x, b along y of the face)"""
    one = np.ones_like(a)
    return [(one, -b, -a), (-one, -b, a), (a, one, b), (a, -one, -b), (a, -b, one), (-a, -b, -one)][f]


def face_coords(size, samples, k, dtype):
    """step 1 for one sub-sample index k: the coordinate of every texel 0 .. size - 1, one rounding"""
    n = size * samples
    num = 2 * (np.arange(size, dtype=np.int64) * samples + k) + 1 - n
    return num.astype(dtype) / dtype(n)


def pano_coords(f, a, b, pw, ph, dtype):
    """steps 2 - 4: (s, t) of the directions of face f at face coordinates a (x) and b (y), arrays of one shape"""
    dx, dy, dz = cube_dir_raw(f, a, b)
    lam = np.where((dx == 0) & (dz == 0), dtype(0), np.arctan2(dx, dz)).astype(dtype)
    theta = np.arctan2(np.sqrt(dx * dx + dz * dz), dy).astype(dtype)
    i2, i1 = dtype(1.0 / (2.0 * np.pi)), dtype(1.0 / np.pi)
    s = (lam * i2 + dtype(0.5)) * dtype(pw) - dtype(0.5)
    t = (theta * i1) * dtype(ph) - dtype(0.5)
    return s, t


def _lerp(p, q, w, dtype):
    """fmaf(w, q - p, p): the difference rounds in dtype, the multiply-add rounds once (float32: through float64, whose 53 bits hold
    the product of two float32 exactly)"""
    d = (q - p).astype(dtype)
    if dtype is np.float64:
        return w * d + p
    return (w.astype(np.float64) * d.astype(np.float64) + p.astype(np.float64)).astype(np.float32)


def equirect_to_cube(pano, size, samples, dtype=np.float64):
    """pano: [ph, pw, >= 3] (alpha is not read) -> [6, size, size, 4] of dtype, alpha 1"""
    pano = np.asarray(pano)
    ph, pw = pano.shape[:2]
    src = pano[..., :3].astype(dtype)
    out = np.ones((6, size, size, 4), dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(6):
            acc = np.zeros((size, size, 3), dtype=dtype)
            for j in range(samples):
                b = face_coords(size, samples, j, dtype)[:, None] * np.ones((1, size), dtype=dtype)
                for i in range(samples):
                    a = np.ones((size, 1), dtype=dtype) * face_coords(size, samples, i, dtype)[None, :]
                    s, t = pano_coords(f, a, b, pw, ph, dtype)
                    sf, tf = np.floor(s), np.floor(t)
                    fx, fy = ((s - sf).astype(dtype))[..., None], ((t - tf).astype(dtype))[..., None]
                    x0, y0 = sf.astype(np.int64), tf.astype(np.int64)
                    c0, c1 = x0 % pw, (x0 + 1) % pw
                    r0, r1 = np.clip(y0, 0, ph - 1), np.clip(y0 + 1, 0, ph - 1)
                    top = _lerp(src[r0, c0], src[r0, c1], fx, dtype)
                    bot = _lerp(src[r1, c0], src[r1, c1], fx, dtype)
                    acc = (acc + _lerp(top, bot, fy, dtype)).astype(dtype)
            out[f, ..., :3] = acc * dtype(1.0 / (samples * samples))
    return out


def coords(pw, ph, size, samples, dtype):
    """(s, t) of every sub-sample, [6, samples, samples, size, size] each: what a coordinate deviation is measured on"""
    S = np.zeros((6, samples, samples, size, size), dtype=dtype)
    T = np.zeros_like(S)
    for f in range(6):
        for j in range(samples):
            b = face_coords(size, samples, j, dtype)[:, None] * np.ones((1, size), dtype=dtype)
            for i in range(samples):
                a = np.ones((size, 1), dtype=dtype) * face_coords(size, samples, i, dtype)[None, :]
                S[f, j, i], T[f, j, i] = pano_coords(f, a, b, pw, ph, dtype)
    return S, T


def rgbe_decode(rgbe):
    """pbr_rgbe_decode's rule: uint8 [..., 4] -> float32 [..., 4], alpha 1 (e == 0: 0, else mantissa * 2^(e - 136); exact)"""
    rgbe = np.asarray(rgbe, dtype=np.uint8)
    e = rgbe[..., 3].astype(np.int32)
    scale = np.where(e == 0, 0.0, np.ldexp(1.0, e - 136))
    out = np.ones(rgbe.shape[:-1] + (4,), dtype=np.float32)
    out[..., :3] = (rgbe[..., :3].astype(np.float64) * scale[..., None]).astype(np.float32)
    return out
