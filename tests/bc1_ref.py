"""numpy restatement of the BC1 rule and the chain sizes pinned in include/pbr_hip.h (PBR_TEX_BC1_BLOCKS, pbr_bc1_decode,
pbr_texture2d_bytes), written from the format's public definition and independently of csrc/bc1_decode.hpp.

A block is 8 bytes: little-endian uint16 c0, c1 (RGB565) and a little-endian uint32 of 16 2-bit indices, texel (x, y) of the
4 x 4 block at bits 2 (4 y + x).  Endpoints expand by bit replication; c0 > c1: four colours (the thirds, rounded as
(2 a + b + 1) // 3), alpha 255; else three colours ((a + b + 1) // 2) and index 3 = transparent black."""
import numpy as np

STORED = {28: 4, 87: 4, 91: 4, 61: 1}          # DXGI number -> bytes per texel
BC1_FLAG = 0x100
MAX_SIZE = 16384


def level_blocks(w, h):
    return max(1, (w + 3) // 4), max(1, (h + 3) // 4)


def chain_bytes(w, h, mips, fmt):
    """bytes of a chain: decoded (fmt one of STORED) or BC1 (fmt | BC1_FLAG); 0 for a bad description"""
    if fmt & ~(0xFF | BC1_FLAG) or (fmt & 0xFF) not in STORED:
        return 0
    if not (1 <= w <= MAX_SIZE and 1 <= h <= MAX_SIZE and mips >= 1 and (min(w, h) >> (mips - 1)) >= 1):
        return 0
    total = 0
    for l in range(mips):
        if fmt & BC1_FLAG:
            bw, bh = level_blocks(w >> l, h >> l)
            total += 8 * bw * bh
        else:
            total += (w >> l) * (h >> l) * STORED[fmt]
    return total


def palette(c0, c1):
    """c0, c1: integer arrays of RGB565 endpoints -> [..., 4 colours, 4 channels RGBA] int64"""
    def chan(c):
        r, g, b = (c >> 11) & 31, (c >> 5) & 63, c & 31
        return np.stack([r * 8 + r // 4, g * 4 + g // 16, b * 8 + b // 4], axis=-1)
    c0, c1 = np.asarray(c0, np.int64), np.asarray(c1, np.int64)
    a, b = chan(c0), chan(c1)
    pal = np.zeros(c0.shape + (4, 4), np.int64)
    pal[..., 0, :3], pal[..., 1, :3] = a, b
    pal[..., :, 3] = 255
    four = c0 > c1
    pal[four, 2, :3] = ((2 * a + b + 1) // 3)[four]
    pal[four, 3, :3] = ((a + 2 * b + 1) // 3)[four]
    pal[~four, 2, :3] = ((a + b + 1) // 2)[~four]
    pal[~four, 3, :] = 0
    return pal


def decode_level(blocks, w, h):
    """the BC1 blocks (uint8, row-major) of a w x h level -> RGBA uint8 [h, w, 4]"""
    bw, bh = level_blocks(w, h)
    b = np.asarray(blocks, np.uint8).reshape(bh, bw, 8).astype(np.int64)
    pal = palette(b[..., 0] + 256 * b[..., 1], b[..., 2] + 256 * b[..., 3])
    bits = b[..., 4] + (b[..., 5] << 8) + (b[..., 6] << 16) + (b[..., 7] << 24)
    full = np.zeros((4 * bh, 4 * bw, 4), np.uint8)
    by, bx = np.mgrid[0:bh, 0:bw]
    for y in range(4):
        for x in range(4):
            idx = (bits >> (2 * (4 * y + x))) & 3
            full[y::4, x::4] = pal[by, bx, idx]
    return full[:h, :w]


def stored(rgba, fmt):
    """RGBA texels -> the stored format's bytes: 28 R, G, B, A; 87 / 91 B, G, R, A; 61 R"""
    if fmt == 28:
        return rgba
    if fmt in (87, 91):
        return rgba[..., [2, 1, 0, 3]]
    if fmt == 61:
        return rgba[..., 0]
    raise ValueError(f"format {fmt}")


def decode_chain(blocks, w, h, mips, fmt):
    """a whole BC1 chain -> its levels in the stored format (uint8 [h_l, w_l, 4], R8: [h_l, w_l])"""
    blocks = np.asarray(blocks, np.uint8).reshape(-1)
    assert blocks.size == chain_bytes(w, h, mips, fmt | BC1_FLAG), (blocks.size, w, h, mips)
    levels, o = [], 0
    for l in range(mips):
        lw, lh = w >> l, h >> l
        bw, bh = level_blocks(lw, lh)
        levels.append(np.ascontiguousarray(stored(decode_level(blocks[o:o + 8 * bw * bh], lw, lh), fmt)))
        o += 8 * bw * bh
    return levels


def level_offset(w, h, l):
    """byte offset of level l in a BC1 chain"""
    return sum(8 * level_blocks(w >> i, h >> i)[0] * level_blocks(w >> i, h >> i)[1] for i in range(l))
