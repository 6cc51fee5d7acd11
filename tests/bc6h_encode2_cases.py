"""Seeded inputs of the two-region BC6H encoder's tests (tests/test_bc6h_encode2_cpu.py, tests/test_gpu_bc6h_encode2.py): name ->
(level 0 float32 [6, s, s, 3], level count).  Together with their box chains they reach all fourteen modes; the tests assert it."""
import os

import numpy as np

import bc6h_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SPECIALS = np.float32([np.nan, np.inf, -np.inf, -1.0, -0.0, 1e9, 65504.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 1.0 + 3 * 2.0 ** -11,
                       6e-8, 3e-5, 2.0 ** -25, 65519.0])
ALL_MODES = tuple(sorted(bc6h_ref.MODES))


def smooth_level0():
    """level 0 of the fixture's analytic sky (gradient + a sun lobe of about 50), float32 [6, 32, 32, 3]"""
    return dict(np.load(os.path.join(HERE, "golden", "sky_bc6h.npz"), allow_pickle=False))["smooth_level0"]


def heavy():
    return (np.random.default_rng(16).random((6, 16, 16, 3)) ** 4 * 200).astype(np.float32)


def per_block(a):
    """[6, n, n, c] per block -> [6, 4 n, 4 n, c] per texel"""
    return np.repeat(np.repeat(a, 4, axis=1), 4, axis=2)


def scaled(seed, amp_scale=(1.0, 1.0, 1.0), size=64):
    """per block and channel a base level U^3 50 and an amplitude U^2: texel = base (1 + 0.6 amp U)"""
    rng, n = np.random.default_rng(seed), size // 4
    base = per_block(rng.random((6, n, n, 3)) ** 3 * 50)
    amp = per_block(rng.random((6, n, n, 3)) ** 2 * np.array(amp_scale))
    return (base * (1 + 0.6 * amp * rng.random((6, size, size, 3)))).astype(np.float32)


def planted(seed, size=64):
    """per block a random shape whose second region is the first times a jump: two populations, each with its own spread"""
    rng, n = np.random.default_rng(seed), size // 4
    base = per_block(2.0 ** rng.uniform(-6, 8, (6, n, n, 3)))
    spread = per_block(2.0 ** rng.uniform(-7, 1.5, (6, n, n, 3)))
    jump = per_block(2.0 ** rng.uniform(-2, 2, (6, n, n, 3)))
    shape = rng.integers(0, 32, (6, n, n))
    second = bc6h_ref.REGION[shape].reshape(6, n, n, 4, 4).transpose(0, 1, 3, 2, 4).reshape(6, size, size, 1)
    return (base * np.where(second == 1, jump, 1.0) * (1 + spread * rng.random((6, size, size, 3)))).astype(np.float32)


def shape_blocks(lo, hi):
    """32 blocks, one per shape, float32 [32, 16, 3] (texels row-major): two gentle ramps, region 1's around hi, region 0's around lo"""
    y, x = np.divmod(np.arange(16), 4)
    r0 = lo * (1 + 0.02 * x[:, None] * np.array([1, 1.5, 2]) + 0.03 * y[:, None] * np.array([1, 1, 1.2]))
    r1 = hi * (1 + 0.04 * x[:, None] * np.array([1, 0.9, 0.7]) + 0.03 * y[:, None] * np.array([1, 0.8, 0.5]))
    return np.where(bc6h_ref.REGION[:, :, None] == 1, r1[None], r0[None]).astype(np.float32)


def rgba(level0_rgb):
    a = np.ones(level0_rgb.shape[:3] + (4,), np.float32)
    a[..., :3] = level0_rgb
    return a


def noise(size, seed):
    rng = np.random.default_rng(seed)
    lv = (rng.random((6, size, size, 3)) ** 4 * 200).astype(np.float32)
    face = lv[3].reshape(-1)
    face[rng.permutation(face.size)[:len(SPECIALS)]] = SPECIALS
    return lv


def cubes():
    """name -> (level 0 float32 [6, s, s, 3], level count)"""
    smooth = smooth_level0()
    return {
        "smooth 32^2 x 6": (smooth, 6),
        "smooth crop 12^2 x 4": (np.ascontiguousarray(smooth[:, :12, :12]), 4),
        "heavy 16^2 x 5": (heavy(), 5),
        "scaled 64^2 x 2": (scaled(31), 2),
        "scaled blue 64^2 x 1": (scaled(32, (0.3, 0.3, 2.5)), 1),
        "planted 64^2 x 2": (planted(33), 2),
        "noise 4^2 x 3": (noise(4, 34), 3),
        "noise 8^2 x 4": (noise(8, 35), 4),
    }
