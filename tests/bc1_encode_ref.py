"""numpy restatement of the BC1 encoding rule pinned in include/pbr_hip.h (pbr_bc1_encode), written from the header text and
independently of csrc/texture2d.hip; the decode side (palette, chain sizes) is tests/bc1_ref.py.

Everything is integer arithmetic (int64 here; the header states that 32 bits suffice), `//` is floor division as the header
demands, and a texel outside its level takes no part in any minimum, maximum or sum and gets index 0."""
import numpy as np

import bc1_ref

WEIGHT_A = np.array([3, 0, 2, 1], np.int64)      # the weight of endpoint A (c0) in palette entry 0 .. 3, in thirds
REFINEMENTS = 3


def rgb_of(texels, fmt):
    """stored texels of a level (uint8 [h, w, 4], R8: [h, w]) -> [h, w, 3] int64 (r, g, b)"""
    t = np.asarray(texels, np.uint8).astype(np.int64)
    if fmt == 28:
        return t[..., :3]
    if fmt in (87, 91):
        return t[..., [2, 1, 0]]
    if fmt == 61:
        return np.stack([t, t, t], axis=-1)
    raise ValueError(f"format {fmt}")


def blocks_of(rgb, outside=0):
    """[h, w, 3] -> ([blocks, 16, 3] texels with texel (x, y) of a block at 4 y + x, [blocks, 16] bool: the texel is in the level).
    outside: what the texels of the blocks that lie outside the level hold (a value or a [4 bh, 4 bw, 3] array); by the rule it
    cannot matter."""
    h, w, _ = rgb.shape
    bw, bh = bc1_ref.level_blocks(w, h)
    full = np.zeros((4 * bh, 4 * bw, 3), np.int64)
    full[:] = outside
    inside = np.zeros((4 * bh, 4 * bw), bool)
    full[:h, :w], inside[:h, :w] = rgb, True
    x = full.reshape(bh, 4, bw, 4, 3).transpose(0, 2, 1, 3, 4).reshape(-1, 16, 3)
    m = inside.reshape(bh, 4, bw, 4).transpose(0, 2, 1, 3).reshape(-1, 16)
    return x, m


def quantise(c):
    """[..., 3] 8-bit channels -> RGB565 words"""
    return (((31 * c[..., 0] + 127) // 255) << 11) | (((63 * c[..., 1] + 127) // 255) << 5) | ((31 * c[..., 2] + 127) // 255)


def fit(x, m, ca, cb):
    """the fit of the pairs (ca, cb) to the blocks: (c0, c1, indices [blocks, 16], error [blocks])"""
    c0, c1 = np.maximum(ca, cb), np.minimum(ca, cb)
    pal = bc1_ref.palette(c0, c1)[..., :3]                                   # [blocks, 4, 3]
    d = ((x[:, :, None, :] - pal[:, None, :, :]) ** 2).sum(-1)               # [blocks, 16, 4]
    idx = d.argmin(-1)                                                       # the first minimum: the lowest index on ties
    idx[c0 == c1] = 0
    idx[~m] = 0
    err = (np.take_along_axis(d, idx[..., None], -1)[..., 0] * m).sum(1)
    return c0, c1, idx, err


def encode_rgb(rgb, outside=0):
    """one level, [h, w, 3] -> its BC1 blocks (uint8, row-major blocks of 8 bytes)"""
    x, m = blocks_of(np.asarray(rgb).astype(np.int64), outside)
    n = m.sum(1)
    lo = np.where(m[..., None], x, 255).min(1)
    hi = np.where(m[..., None], x, 0).max(1)
    dom = (hi - lo).argmax(1)                                                # the first of r, g, b on ties
    xm = x * m[..., None]
    xd = np.take_along_axis(xm, dom[:, None, None], 2)[..., 0]               # [blocks, 16]
    cov = n[:, None] * (xm * xd[..., None]).sum(1) - xm.sum(1) * xd.sum(1)[:, None]
    a, b = np.where(cov < 0, lo, hi), np.where(cov < 0, hi, lo)
    c0, c1, idx, err = fit(x, m, quantise(a), quantise(b))
    live = np.ones(len(x), bool)                                             # blocks that have not stopped
    for _ in range(REFINEMENTS):
        wa = WEIGHT_A[idx] * m
        wb = (3 - WEIGHT_A[idx]) * m
        saa, sbb, sab = (wa * wa).sum(1), (wb * wb).sum(1), (wa * wb).sum(1)
        sax, sbx = (wa[..., None] * x).sum(1), (wb[..., None] * x).sum(1)
        det = saa * sbb - sab * sab
        live &= det != 0
        dd = np.where(det != 0, det, 1)[:, None]
        a = np.clip((6 * (sbb[:, None] * sax - sab[:, None] * sbx) + dd) // (2 * dd), 0, 255)
        b = np.clip((6 * (saa[:, None] * sbx - sab[:, None] * sax) + dd) // (2 * dd), 0, 255)
        n0, n1, nidx, nerr = fit(x, m, quantise(a), quantise(b))
        live &= nerr < err
        c0, c1, err = np.where(live, n0, c0), np.where(live, n1, c1), np.where(live, nerr, err)
        idx = np.where(live[:, None], nidx, idx)
    bits = (idx << (2 * np.arange(16))).sum(1)
    out = np.zeros((len(x), 8), np.uint8)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = c0 & 255, c0 >> 8, c1 & 255, c1 >> 8
    for i in range(4):
        out[:, 4 + i] = (bits >> (8 * i)) & 255
    return out.reshape(-1)


def encode_level(texels, fmt):
    """one level in the stored format fmt -> its blocks"""
    return encode_rgb(rgb_of(texels, fmt))


def encode_chain(levels, fmt):
    """the levels of a chain in the stored format (scene.mip_chain's list) -> the BC1 chain's bytes (PBR_TEX_BC1_BLOCKS layout)"""
    return np.concatenate([encode_level(lv, fmt) for lv in levels])


def squared_error(blocks, rgb):
    """total squared error over r, g, b of the pinned decode of `blocks` against the [h, w, 3] image"""
    h, w, _ = rgb.shape
    d = bc1_ref.decode_level(blocks, w, h)[..., :3].astype(np.int64) - np.asarray(rgb).astype(np.int64)
    return int((d * d).sum())
