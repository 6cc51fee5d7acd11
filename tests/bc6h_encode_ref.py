"""numpy restatement of the BC6H_UF16 ENCODING rule pinned in include/pbr_hip.h (pbr_bc6h_encode_cube), written from that text and
independently of csrc/bc6h_encode.hip: whole levels at a time, one array axis per block, Python's floor division, and the block's
bits placed through bc6h_ref.header_bits (the decode restatement's own table of the header), not through the kernel's shifts.
Everything after half_code is int64.  encode_* return the blocks together with what the rule PREDICTS for them (squared error in
half-code space, mode), so a test can hold the prediction to a decoder the encoder did not write (bc6h_ref.decode_blocks)."""
import numpy as np

import bc6h_ref

W4 = bc6h_ref.WEIGHTS4
# mode, endpoint bits, delta bits, transformed — in the order the rule tries them
ONE_REGION = ((0x0F, 16, 4, True), (0x0B, 12, 8, True), (0x07, 11, 9, True), (0x03, 10, 10, False))
HEADER = {m: bc6h_ref.header_bits(m) for m, _, _, _ in ONE_REGION}


def half_code(x):
    """fp32 -> the IEEE half bit pattern of clamp(x, 0, 65504) rounded to nearest even; NaN and everything <= 0 (-0.0 too) give 0"""
    x = np.asarray(x, np.float32)
    v = np.where(np.isnan(x) | (x <= 0), np.float32(0), np.minimum(x, np.float32(65504.0))).astype(np.float32)
    return v.astype(np.float16).view(np.uint16).astype(np.int64)


def level_texels(rgb):
    """a level float32 [s, s, >= 3] -> (half codes int64 [blocks, 16, 3], inside bool [blocks, 16]); blocks row-major, texels row-major"""
    s = rgb.shape[0]
    bw = bc6h_ref.level_blocks(s)
    h = np.zeros((4 * bw, 4 * bw, 3), np.int64)
    h[:s, :s] = half_code(np.asarray(rgb)[..., :3])
    inside = np.zeros((4 * bw, 4 * bw), bool)
    inside[:s, :s] = True
    return (h.reshape(bw, 4, bw, 4, 3).transpose(0, 2, 1, 3, 4).reshape(bw * bw, 16, 3),
            inside.reshape(bw, 4, bw, 4).transpose(0, 2, 1, 3).reshape(bw * bw, 16))


def fit(a, b, h, inside):
    """16-bit endpoint triples a, b [n, 3] -> (indices [n, 16], error [n])"""
    w = W4[None, :, None]
    pal = ((((a[:, None, :] * (64 - w) + b[:, None, :] * w + 32) >> 6) * 31) >> 6)          # [n, k, c]
    d = ((pal[:, None, :, :] - h[:, :, None, :]) ** 2).sum(axis=-1)                          # [n, texel, k]
    idx = d.argmin(axis=-1)                                                                  # the first minimum: the lowest k
    best = np.take_along_axis(d, idx[..., None], axis=-1)[..., 0]
    assert best.max(initial=0) < 2 ** 32
    return np.where(inside, idx, 0), np.where(inside, best, 0).sum(axis=1)


def encode_blocks(h, inside):
    """half codes [n, 16, 3], inside [n, 16] -> (blocks uint8 [n, 16], predicted error int64 [n], mode int64 [n])"""
    h, inside = np.asarray(h, np.int64), np.asarray(inside, bool)
    nb = len(h)
    m3 = inside[..., None]
    t = (64 * h + 30) // 31
    lo = np.where(m3, t, 1 << 20).min(axis=1)
    hi = np.where(m3, t, -1).max(axis=1)
    dom = (hi - lo).argmax(axis=1)                               # the first of r, g, b on ties
    tz = np.where(m3, t, 0)
    td = np.take_along_axis(tz, dom[:, None, None], axis=2)      # [n, 16, 1]
    n = inside.sum(axis=1)[:, None]
    cov = n * (tz * td).sum(axis=1) - tz.sum(axis=1) * td.sum(axis=1)
    A, B = np.where(cov < 0, lo, hi), np.where(cov < 0, hi, lo)
    idx, err = fit(A, B, h, inside)

    going = np.ones(nb, bool)
    for _ in range(2):
        al = np.where(inside, 64 - W4[idx], 0)
        be = np.where(inside, W4[idx], 0)
        saa, sbb, sab = (al * al).sum(axis=1), (be * be).sum(axis=1), (al * be).sum(axis=1)
        sat, sbt = (al[..., None] * tz).sum(axis=1), (be[..., None] * tz).sum(axis=1)
        det = saa * sbb - sab * sab
        assert (det >= 0).all()
        can = going & (det != 0)
        dd = np.where(can, det, 1)[:, None]
        A2 = np.clip((128 * (sbb[:, None] * sat - sab[:, None] * sbt) + dd) // (2 * dd), 0, 65535)
        B2 = np.clip((128 * (saa[:, None] * sbt - sab[:, None] * sat) + dd) // (2 * dd), 0, 65535)
        idx2, err2 = fit(A2, B2, h, inside)
        better = can & (err2 < err)
        A, B = np.where(better[:, None], A2, A), np.where(better[:, None], B2, B)
        idx, err = np.where(better[:, None], idx2, idx), np.where(better, err2, err)
        going = better

    best_err = np.full(nb, np.iinfo(np.int64).max)
    best_mode = np.zeros(nb, np.int64)
    best_a, best_b, best_idx = np.zeros((nb, 3), np.int64), np.zeros((nb, 3), np.int64), np.zeros((nb, 16), np.int64)
    for mode, bits, dbits, transformed in ONE_REGION:
        qa, qb = A >> (16 - bits), B >> (16 - bits)
        mi, me = fit(bc6h_ref.unquantize(qa, bits), bc6h_ref.unquantize(qb, bits), h, inside)
        flip = mi[:, 0] >= 8
        qa, qb = np.where(flip[:, None], qb, qa), np.where(flip[:, None], qa, qb)
        mi = np.where(flip[:, None] & inside, 15 - mi, mi)
        delta = qb - qa
        ok = ((delta >= -(1 << (dbits - 1))) & (delta < (1 << (dbits - 1)))).all(axis=1) if transformed else np.ones(nb, bool)
        take = ok & (me < best_err)                              # strictly: the earlier mode keeps a tie
        best_err, best_mode = np.where(take, me, best_err), np.where(take, mode, best_mode)
        best_a, best_b = np.where(take[:, None], qa, best_a), np.where(take[:, None], qb, best_b)
        best_idx = np.where(take[:, None], mi, best_idx)
    assert (best_mode != 0).all() and (best_idx[:, 0] < 8).all()

    bits128 = np.zeros((nb, 128), np.uint8)
    for mode, bits, dbits, transformed in ONE_REGION:
        sel = np.nonzero(best_mode == mode)[0]
        if not len(sel):
            continue
        for k in range(5):
            bits128[sel, k] = (mode >> k) & 1
        second = (best_b[sel] - best_a[sel]) & ((1 << dbits) - 1) if transformed else best_b[sel]      # two's complement of the width
        field = {c + "0": best_a[sel, ci] for ci, c in enumerate("rgb")}
        field.update({c + "1": second[:, ci] for ci, c in enumerate("rgb")})
        for pos, name, k in HEADER[mode]:
            bits128[sel, pos] = (field[name] >> k) & 1
    pos = 65
    for tx in range(16):
        for k in range(3 if tx == 0 else 4):
            bits128[:, pos] = (best_idx[:, tx] >> k) & 1
            pos += 1
    assert pos == 128
    return np.packbits(bits128, axis=1, bitorder="little"), best_err, best_mode


def encode_level(rgb):
    """a level float32 [s, s, >= 3] -> (blocks uint8 [blocks, 16] row-major, predicted error [blocks], mode [blocks])"""
    return encode_blocks(*level_texels(rgb))


def cube_levels(cube, size, mip_levels):
    """the pbr_cube_f32 layout (float32 [texels, 4]: mips concatenated, six faces per mip) -> levels[l][f] float32 [s, s, 4]"""
    cube = np.asarray(cube, np.float32).reshape(-1, 4)
    out, o = [], 0
    for l in range(mip_levels):
        s = max(size >> l, 1)
        out.append([cube[o + f * s * s:o + (f + 1) * s * s].reshape(s, s, 4) for f in range(6)])
        o += 6 * s * s
    assert o == len(cube)
    return out


def encode_cube(cube, size, mip_levels, chunk=1024):
    """the pbr_cube_f32 chain -> six face chains (uint8, bc6h_ref.chain_bytes each): what pbr_bc6h_encode_cube writes"""
    faces = [[] for _ in range(6)]
    for level in cube_levels(cube, size, mip_levels):
        for f in range(6):
            h, inside = level_texels(level[f])
            for o in range(0, len(h), chunk):                    # (the fit's [n, 16, 16, 3] temporaries: bounded)
                faces[f].append(encode_blocks(h[o:o + chunk], inside[o:o + chunk])[0].reshape(-1))
    return [np.concatenate(f) for f in faces]


def box_mips(level0, mip_levels):
    """level 0 float32 [6, s, s, c] -> its levels, each the fp32 mean of the 2 x 2 texels above (bc6h_ref.encode_mode3_chain's)"""
    out, img = [np.asarray(level0, np.float32)], np.asarray(level0, np.float32)
    for _ in range(1, mip_levels):
        s = img.shape[1] // 2
        img = img[:, :2 * s, :2 * s].reshape(6, s, 2, s, 2, -1).mean(axis=(2, 4), dtype=np.float32)
        out.append(img)
    return out
