"""numpy restatement of the BC6H_UF16 rule pinned in include/pbr_hip.h (pbr_bc6h_decode_cube), written from the format's public
definition and independently of csrc/bc6h_decode.hip, plus the test-side block packers: a generic one (any mode, from its field
values), a deliberately simple single-mode encoder (mode 0x03) that exists only to make smooth test skies, and a constant-colour
packer (mode 0x0f).  None of the packers is a product feature.

A block is 16 bytes, read as 128 bits, LSB first.  The mode is bits 0-1 if they are 0 or 1, otherwise bits 0-4; the header fields
follow in the order of MODES below; two-region modes end with a 5-bit partition at bits 77-81 and 46 index bits from bit 82, one-
region modes hold 63 index bits from bit 65.  weight_round is the rounding term of the interpolation: 32 is the pinned rule
(DirectXTex's BC67_WEIGHT_ROUND), 0 is what Pillow's decoder computes."""
import re

import numpy as np

MAX_SIZE = 8192
CHANNELS = ("r", "g", "b")
FIELDS = [c + str(i) for i in range(4) for c in CHANNELS]       # r0 g0 b0 r1 ... b3

# mode -> (endpoint bits, (delta bits r, g, b), transformed, two regions, the header after the mode bits)
# x[a:b] with a > b stores bit b first; with a < b (r0[10:11], r0[10:15]) the HIGH bit first
MODES = {
    0x00: (10, (5, 5, 5), True, True, "g2[4] b2[4] b3[4] r0[9:0] g0[9:0] b0[9:0] r1[4:0] g3[4] g2[3:0] g1[4:0] b3[0] g3[3:0] b1[4:0] b3[1] b2[3:0] r2[4:0] b3[2] r3[4:0] b3[3]"),
    0x01: (7, (6, 6, 6), True, True, "g2[5] g3[4] g3[5] r0[6:0] b3[0] b3[1] b2[4] g0[6:0] b2[5] b3[2] g2[4] b0[6:0] b3[3] b3[5] b3[4] r1[5:0] g2[3:0] g1[5:0] g3[3:0] b1[5:0] b2[3:0] r2[5:0] r3[5:0]"),
    0x02: (11, (5, 4, 4), True, True, "r0[9:0] g0[9:0] b0[9:0] r1[4:0] r0[10] g2[3:0] g1[3:0] g0[10] b3[0] g3[3:0] b1[3:0] b0[10] b3[1] b2[3:0] r2[4:0] b3[2] r3[4:0] b3[3]"),
    0x06: (11, (4, 5, 4), True, True, "r0[9:0] g0[9:0] b0[9:0] r1[3:0] r0[10] g3[4] g2[3:0] g1[4:0] g0[10] g3[3:0] b1[3:0] b0[10] b3[1] b2[3:0] r2[3:0] b3[0] b3[2] r3[3:0] g2[4] b3[3]"),
    0x0a: (11, (4, 4, 5), True, True, "r0[9:0] g0[9:0] b0[9:0] r1[3:0] r0[10] b2[4] g2[3:0] g1[3:0] g0[10] b3[0] g3[3:0] b1[4:0] b0[10] b2[3:0] r2[3:0] b3[1] b3[2] r3[3:0] b3[4] b3[3]"),
    0x0e: (9, (5, 5, 5), True, True, "r0[8:0] b2[4] g0[8:0] g2[4] b0[8:0] b3[4] r1[4:0] g3[4] g2[3:0] g1[4:0] b3[0] g3[3:0] b1[4:0] b3[1] b2[3:0] r2[4:0] b3[2] r3[4:0] b3[3]"),
    0x12: (8, (6, 5, 5), True, True, "r0[7:0] g3[4] b2[4] g0[7:0] b3[2] g2[4] b0[7:0] b3[3] b3[4] r1[5:0] g2[3:0] g1[4:0] b3[0] g3[3:0] b1[4:0] b3[1] b2[3:0] r2[5:0] r3[5:0]"),
    0x16: (8, (5, 6, 5), True, True, "r0[7:0] b3[0] b2[4] g0[7:0] g2[5] g2[4] b0[7:0] g3[5] b3[4] r1[4:0] g3[4] g2[3:0] g1[5:0] g3[3:0] b1[4:0] b3[1] b2[3:0] r2[4:0] b3[2] r3[4:0] b3[3]"),
    0x1a: (8, (5, 5, 6), True, True, "r0[7:0] b3[1] b2[4] g0[7:0] b2[5] g2[4] b0[7:0] b3[5] b3[4] r1[4:0] g3[4] g2[3:0] g1[4:0] b3[0] g3[3:0] b1[5:0] b2[3:0] r2[4:0] b3[2] r3[4:0] b3[3]"),
    0x1e: (6, (6, 6, 6), False, True, "r0[5:0] g3[4] b3[0] b3[1] b2[4] g0[5:0] g2[5] b2[5] b3[2] g2[4] b0[5:0] g3[5] b3[3] b3[5] b3[4] r1[5:0] g2[3:0] g1[5:0] g3[3:0] b1[5:0] b2[3:0] r2[5:0] r3[5:0]"),
    0x03: (10, (10, 10, 10), False, False, "r0[9:0] g0[9:0] b0[9:0] r1[9:0] g1[9:0] b1[9:0]"),
    0x07: (11, (9, 9, 9), True, False, "r0[9:0] g0[9:0] b0[9:0] r1[8:0] r0[10] g1[8:0] g0[10] b1[8:0] b0[10]"),
    0x0b: (12, (8, 8, 8), True, False, "r0[9:0] g0[9:0] b0[9:0] r1[7:0] r0[10:11] g1[7:0] g0[10:11] b1[7:0] b0[10:11]"),
    0x0f: (16, (4, 4, 4), True, False, "r0[9:0] g0[9:0] b0[9:0] r1[3:0] r0[10:15] g1[3:0] g0[10:15] b1[3:0] b0[10:15]"),
}
RESERVED = (0x13, 0x17, 0x1b, 0x1f)
# texel 0 first, '1' = the second endpoint pair (e2 / e3)
PARTITIONS = """
0011001100110011 0001000100010001 0111011101110111 0001001100110111 0000000100010011 0011011101111111 0001001101111111 0000000100110111
0000000000010011 0011011111111111 0000000101111111 0000000000010111 0001011111111111 0000000011111111 0000111111111111 0000000000001111
0000100011101111 0111000100000000 0000000010001110 0111001100010000 0011000100000000 0000100011001110 0000000010001100 0111001100110001
0011000100010000 0000100010001100 0110011001100110 0011011001101100 0001011111101000 0000111111110000 0111000110001110 0011100110011100
""".split()
ANCHOR = [15] * 17 + [2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2]
WEIGHTS3 = np.array([0, 9, 18, 27, 37, 46, 55, 64], np.int64)
WEIGHTS4 = np.array([0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64], np.int64)
REGION = np.array([[int(c) for c in p] for p in PARTITIONS], np.int64)      # [shape, texel]
assert REGION.shape == (32, 16) and len(ANCHOR) == 32
assert all(REGION[s, 0] == 0 and REGION[s, ANCHOR[s]] == 1 and REGION[s, :ANCHOR[s]].max() >= 0 for s in range(32))


def header_bits(mode):
    """the header of a mode as a list of (block bit, field, field bit), in file order"""
    out, pos = [], 2 if mode < 2 else 5
    for token in MODES[mode][4].split():
        m = re.fullmatch(r"([rgb][0-3])\[(\d+)(?::(\d+))?\]", token)
        name, a, b = m.group(1), int(m.group(2)), m.group(3)
        if b is None:
            order = [a]
        elif a > int(b):
            order = list(range(int(b), a + 1))            # bit b first
        else:
            order = list(range(int(b), a - 1, -1))        # the high bit first
        for k in order:
            out.append((pos, name, k))
            pos += 1
    assert pos == (77 if MODES[mode][3] else 65), (hex(mode), pos)
    return out


for _m, (_n, _d, _t, _two, _s) in MODES.items():             # every field bit of every mode is stored exactly once
    _seen = sorted((f, k) for _, f, k in header_bits(_m))
    _want = sorted([(c + "0", k) for c in CHANNELS for k in range(_n)]
                   + [(c + str(i), k) for ci, c in enumerate(CHANNELS) for i in range(1, 4 if _two else 2) for k in range(_d[ci])])
    assert _seen == _want, hex(_m)


def level_blocks(s):
    return max(1, (s + 3) // 4)


def chain_bytes(size, mips):
    """bytes of one face's chain; 0 for what the decode refuses"""
    size, mips = int(size), int(mips)
    if not (1 <= size <= MAX_SIZE) or size % 4 or not (1 <= mips <= size.bit_length()):
        return 0
    return sum(16 * level_blocks(size >> l) ** 2 for l in range(mips))


def block_modes(blocks):
    b0 = np.asarray(blocks, np.uint8).reshape(-1, 16)[:, 0].astype(np.int64)
    return np.where((b0 & 3) < 2, b0 & 3, b0 & 31)


def unquantize(x, n):
    if n >= 15:
        return x
    full = (1 << n) - 1
    return np.where(x == 0, 0, np.where(x == full, 0xFFFF, ((x << 15) + 0x4000) >> (n - 1)))


def decode_blocks(blocks, weight_round=32):
    """n blocks (uint8 [n, 16]) -> the half bit patterns of their texels, int64 [n, 16 texels, 3]"""
    blocks = np.asarray(blocks, np.uint8).reshape(-1, 16)
    n = len(blocks)
    bits = np.unpackbits(blocks, axis=1, bitorder="little").astype(np.int64)      # [n, 128]
    mode = block_modes(blocks)
    out = np.zeros((n, 16, 3), np.int64)                                          # reserved modes stay 0
    pow2 = 1 << np.arange(64, dtype=np.int64)
    for m, (nb, delta, transformed, two, _) in MODES.items():
        sel = np.nonzero(mode == m)[0]
        if not len(sel):
            continue
        bm = bits[sel]
        f = {name: np.zeros(len(sel), np.int64) for name in FIELDS}
        for pos, name, k in header_bits(m):
            f[name] |= bm[:, pos] << k
        e = np.zeros((len(sel), 4, 3), np.int64)
        for ci, c in enumerate(CHANNELS):
            e[:, 0, ci] = f[c + "0"]
            for i in range(1, 4):
                v = f[c + str(i)]
                if transformed:
                    v = np.where(v >= (1 << (delta[ci] - 1)), v - (1 << delta[ci]), v)     # sign-extend the delta
                    v = (f[c + "0"] + v) & ((1 << nb) - 1)
                e[:, i, ci] = v
        e = unquantize(e, nb)
        if two:
            shape = (bm[:, 77:82] * pow2[:5]).sum(axis=1)
            region, anchor, ib, base, weights = REGION[shape], np.array(ANCHOR)[shape], 3, 82, WEIGHTS3
        else:
            region, anchor, ib, base, weights = np.zeros((len(sel), 16), np.int64), np.full(len(sel), -1), 4, 65, WEIGHTS4
        for t in range(16):
            start = base + ib * t - (1 if t > 0 else 0) - ((anchor >= 0) & (t > anchor))
            width = np.where((t == 0) | (t == anchor), ib - 1, ib)
            idx = np.zeros(len(sel), np.int64)
            for k in range(ib):
                idx |= np.where(k < width, bm[np.arange(len(sel)), np.minimum(start + k, 127)], 0) << k
            w = weights[idx][:, None]
            a = e[np.arange(len(sel)), 2 * region[:, t]]
            b = e[np.arange(len(sel)), 2 * region[:, t] + 1]
            x = (a * (64 - w) + b * w + weight_round) >> 6
            out[sel, t] = (x * 31) >> 6
    return out


def decode_level(blocks, s, weight_round=32):
    """the blocks (row-major) of an s x s level -> float32 [s, s, 4], alpha 1; a block that overhangs keeps its top-left texels"""
    bw = level_blocks(s)
    h = decode_blocks(np.asarray(blocks, np.uint8).reshape(bw * bw, 16), weight_round).reshape(bw, bw, 4, 4, 3)
    full = h.transpose(0, 2, 1, 3, 4).reshape(4 * bw, 4 * bw, 3)[:s, :s]
    out = np.ones((s, s, 4), np.float32)
    out[..., :3] = full.astype(np.uint16).view(np.float16).astype(np.float32)
    return out


def decode(blocks, size, mip_levels, weight_round=32):
    """one face's chain (uint8, levels concatenated) -> its levels, float32 [s_l, s_l, 4]"""
    blocks = np.asarray(blocks, np.uint8).reshape(-1)
    assert blocks.size == chain_bytes(size, mip_levels), (blocks.size, size, mip_levels)
    levels, o = [], 0
    for l in range(mip_levels):
        s = size >> l
        nb = 16 * level_blocks(s) ** 2
        levels.append(decode_level(blocks[o:o + nb], s, weight_round))
        o += nb
    return levels


def decode_cube(faces, size, mip_levels):
    """six face chains -> the pbr_cube_f32 layout (mips concatenated, six faces per mip), float32 [texels, 4]"""
    per_face = [decode(f, size, mip_levels) for f in faces]
    return np.concatenate([per_face[f][l].reshape(-1, 4) for l in range(mip_levels) for f in range(6)])


# ---- packers (test side only) ---------------------------------------------------------------------------------------------
def pack(mode, fields, indices, shape=0):
    """one block from a mode's STORED field values (r0 .. b3 as the header holds them: deltas in two's complement of their width),
    its 16 indices (an anchor's high bit must be 0) and, for the two-region modes, the partition"""
    two = MODES[mode][3]
    bits = np.zeros(128, np.uint8)
    for k in range(2 if mode < 2 else 5):
        bits[k] = (mode >> k) & 1
    for pos, name, k in header_bits(mode):
        bits[pos] = (int(fields.get(name, 0)) >> k) & 1
    ib, pos = (3, 82) if two else (4, 65)
    if two:
        for k in range(5):
            bits[77 + k] = (shape >> k) & 1
    for t in range(16):
        width = ib - 1 if t == 0 or (two and t == ANCHOR[shape]) else ib
        assert 0 <= int(indices[t]) < (1 << width), (t, indices[t])
        for k in range(width):
            bits[pos] = (int(indices[t]) >> k) & 1
            pos += 1
    assert pos == 128
    return np.packbits(bits, bitorder="little")


def pack_mode3(e0, e1, indices):
    """blocks of mode 0x03 (10.10, one region, not transformed): e0, e1 int [n, 3] in 0 .. 1023, indices int [n, 16] with
    indices[:, 0] < 8 -> uint8 [n, 16]"""
    e0, e1, indices = np.asarray(e0, np.int64), np.asarray(e1, np.int64), np.asarray(indices, np.int64)
    assert (indices[:, 0] < 8).all() and indices.max() < 16 and max(e0.max(), e1.max()) < 1024
    bits = np.zeros((len(e0), 128), np.uint8)
    bits[:, 0] = bits[:, 1] = 1                                  # mode 0x03 in bits 0-4
    pos = 5
    for v in (e0[:, 0], e0[:, 1], e0[:, 2], e1[:, 0], e1[:, 1], e1[:, 2]):
        for k in range(10):
            bits[:, pos] = (v >> k) & 1
            pos += 1
    for t in range(16):
        for k in range(3 if t == 0 else 4):
            bits[:, pos] = (indices[:, t] >> k) & 1
            pos += 1
    assert pos == 128
    return np.packbits(bits, axis=1, bitorder="little")


def float_to_half_code(x):
    """fp32 -> the UF16 half bit pattern at or below it (0 .. 0x7BFF)"""
    h = np.clip(np.asarray(x, np.float32), 0.0, 65504.0).astype(np.float16)
    h = np.where(h.astype(np.float32) > x, np.nextafter(h, np.float16(0)), h).astype(np.float16)
    return h.view(np.uint16).astype(np.int64)


def encode_mode3(rgb_f32):
    """a square level float32 [s, s, 3] -> its mode-0x03 blocks (uint8 [blocks, 16], row-major).  Per block: the bounding endpoints per
    channel quantized to 10 bits (floor / ceil), per texel the weight of least squared error in half-code space, and the anchor's high
    bit cleared by swapping the endpoints.  A level that is no multiple of 4 repeats its last row / column into the overhang."""
    s = rgb_f32.shape[0]
    bw = level_blocks(s)
    img = np.pad(np.asarray(rgb_f32, np.float32), ((0, 4 * bw - s), (0, 4 * bw - s), (0, 0)), mode="edge")
    h = float_to_half_code(img).reshape(bw, 4, bw, 4, 3).transpose(0, 2, 1, 3, 4).reshape(bw * bw, 16, 3)
    # a 10-bit endpoint q unquantizes to 64 q + 32 (0 -> 0, 1023 -> 0xFFFF) and a value x finishes as the half code (31 x) >> 6
    x = (h * 64 + 30) // 31                                      # the smallest x that finishes as h
    e0 = np.clip((x.min(axis=1) - 32) // 64, 0, 1023)
    e1 = np.clip(-((32 - x.max(axis=1)) // 64), 0, 1023)
    a, b = unquantize(e0, 10)[:, None, None, :], unquantize(e1, 10)[:, None, None, :]
    w = WEIGHTS4[None, None, :, None]
    cand = (((a * (64 - w) + b * w + 32) >> 6) * 31) >> 6        # [n, 1, 16 weights, 3]
    idx = ((cand - h[:, :, None, :]) ** 2).sum(axis=-1).argmin(axis=-1)
    swap = idx[:, 0] >= 8
    idx = np.where(swap[:, None], 15 - idx, idx)
    e0, e1 = np.where(swap[:, None], e1, e0), np.where(swap[:, None], e0, e1)
    return pack_mode3(e0, e1, idx)


def encode_mode3_chain(level0_rgb, mip_levels):
    """level 0 float32 [s, s, 3] -> one face's chain (2 x 2 box mips of the fp32 image, each level through encode_mode3)"""
    out, img = [], np.asarray(level0_rgb, np.float32)
    for l in range(mip_levels):
        out.append(encode_mode3(img).reshape(-1))
        if l + 1 < mip_levels:
            s = img.shape[0] // 2
            img = img[:2 * s, :2 * s].reshape(s, 2, s, 2, 3).mean(axis=(1, 3), dtype=np.float32)
    return np.concatenate(out)


def pack_constant(c):
    """one block of mode 0x0f whose every texel decodes to the half code c in r, g and b: r0 = ceil(64 c / 31), deltas 0, indices 0"""
    r0 = (64 * int(c) + 30) // 31
    assert r0 < 65536
    return pack(0x0f, {"r0": r0, "g0": r0, "b0": r0}, [0] * 16)


def dds_bc6h(blocks, width, height):
    """an in-memory DDS (DX10 header, DXGI_FORMAT_BC6H_UF16 = 95) around one level of blocks: what a third-party decoder reads"""
    import struct
    blocks = np.asarray(blocks, np.uint8).reshape(-1)
    pf = struct.pack("<II4sIIIII", 32, 0x4, b"DX10", 0, 0, 0, 0, 0)
    head = struct.pack("<IIIIIII44x", 124, 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000, height, width, blocks.size, 0, 1) + pf + \
        struct.pack("<IIIII", 0x1000, 0, 0, 0, 0)
    assert len(head) == 124
    dx10 = struct.pack("<IIIII", 95, 3, 0, 1, 0)
    return b"DDS " + head + dx10 + blocks.tobytes()
