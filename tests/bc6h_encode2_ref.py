"""numpy restatement of the TWO-REGION extension of the BC6H_UF16 encoding rule pinned in include/pbr_hip.h
(pbr_bc6h_encode_cube_ex with PBR_BC6H_ENCODE_TWO_REGION), written from that text and independently of csrc/bc6h_encode_block.hpp:
whole levels at a time, one array axis per block, Python's floor division, the block's bits placed through bc6h_ref.header_bits and
bc6h_ref.pack's layout.  The one-region rule is imported from bc6h_encode_ref, not copied.  encode_* return the blocks together with
what the rule PREDICTS for them (squared error in half-code space, mode) and the shape the search chose — a diagnostic that is
reported even where the one-region block won — so a test can hold the prediction to a decoder the encoder did not write."""
import numpy as np

import bc6h_encode_ref as enc
import bc6h_ref

W3 = bc6h_ref.WEIGHTS3
# the order the rule tries them; endpoint bits, delta bits and `transformed` come from the decode restatement's table
TWO_REGION = (0x00, 0x01, 0x02, 0x06, 0x0A, 0x0E, 0x12, 0x16, 0x1A, 0x1E)
ANCHOR = np.array(bc6h_ref.ANCHOR, np.int64)
assert all(bc6h_ref.MODES[m][3] for m in TWO_REGION) and len(TWO_REGION) == 10


def fit3(e, region, h, inside):
    """e: 16-bit endpoints [n, region, a / b, 3]; region [n, 16] (0 / 1 per texel) -> (indices [n, 16], 0 outside the level;
    error per region [n, 2]): each inside texel takes, of its region's eight palette entries, the one of least squared distance in
    half-code space, the lowest index on ties"""
    w = W3[None, None, :, None]
    pal = ((((e[:, :, 0, None, :] * (64 - w) + e[:, :, 1, None, :] * w + 32) >> 6) * 31) >> 6)      # [n, region, k, c]
    mine = np.take_along_axis(pal, region[:, :, None, None], axis=1)                                    # [n, texel, k, c]
    d = ((mine - h[:, :, None, :]) ** 2).sum(axis=-1)
    idx = d.argmin(axis=-1)                                                                             # the first minimum
    best = np.take_along_axis(d, idx[..., None], axis=-1)[..., 0]
    assert best.max(initial=0) < 2 ** 32
    err = np.stack([np.where(inside & (region == r), best, 0).sum(axis=1) for r in (0, 1)], axis=1)
    return np.where(inside, idx, 0), err


def start(t, mask):
    """the bounding-box start over the texels of mask [n, 16]: (A, B) [n, 3]; an empty mask gives 0, 0"""
    m3 = mask[..., None]
    lo = np.where(m3, t, 1 << 20).min(axis=1)
    hi = np.where(m3, t, -1).max(axis=1)
    dom = (hi - lo).argmax(axis=1)                               # the first of r, g, b on ties
    tz = np.where(m3, t, 0)
    td = np.take_along_axis(tz, dom[:, None, None], axis=2)
    n = mask.sum(axis=1)[:, None]
    cov = n * (tz * td).sum(axis=1) - tz.sum(axis=1) * td.sum(axis=1)
    some = mask.any(axis=1)[:, None]
    return np.where(some, np.where(cov < 0, lo, hi), 0), np.where(some, np.where(cov < 0, hi, lo), 0)


def starts(t, inside, region):
    """-> endpoints [n, 2, 2, 3] of both regions' starts"""
    a0, b0 = start(t, inside & (region == 0))
    a1, b1 = start(t, inside & (region == 1))
    return np.stack([np.stack([a0, b0], axis=1), np.stack([a1, b1], axis=1)], axis=1)


def encode_blocks(h, inside):
    """half codes [n, 16, 3], inside [n, 16] -> (blocks uint8 [n, 16], predicted error int64 [n], mode int64 [n], searched shape [n])"""
    h, inside = np.asarray(h, np.int64), np.asarray(inside, bool)
    nb = len(h)
    one_blocks, one_err, one_mode = enc.encode_blocks(h, inside)                 # step 1
    t = (64 * h + 30) // 31

    # step 3: the shape of least estimate, the lowest number on ties
    best_est, shape = np.full(nb, np.iinfo(np.int64).max), np.zeros(nb, np.int64)
    for s in range(32):
        region = np.broadcast_to(bc6h_ref.REGION[s], (nb, 16))
        est = fit3(starts(t, inside, region), region, h, inside)[1].sum(axis=1)
        take = est < best_est
        best_est, shape = np.where(take, est, best_est), np.where(take, s, shape)

    # step 4: refine the chosen shape, region by region
    region = bc6h_ref.REGION[shape]
    e = starts(t, inside, region)
    idx, err = fit3(e, region, h, inside)
    assert np.array_equal(err.sum(axis=1), best_est)
    going = np.ones((nb, 2), bool)
    for _ in range(2):
        e2 = e.copy()
        can = going.copy()
        for r in (0, 1):
            m = inside & (region == r)
            al, be = np.where(m, 64 - W3[idx], 0), np.where(m, W3[idx], 0)
            tz = np.where(m[..., None], t, 0)
            saa, sbb, sab = (al * al).sum(axis=1), (be * be).sum(axis=1), (al * be).sum(axis=1)
            sat, sbt = (al[..., None] * tz).sum(axis=1), (be[..., None] * tz).sum(axis=1)
            det = saa * sbb - sab * sab
            assert (det >= 0).all()
            can[:, r] &= det != 0
            dd = np.where(det != 0, det, 1)[:, None]
            a2 = np.clip((128 * (sbb[:, None] * sat - sab[:, None] * sbt) + dd) // (2 * dd), 0, 65535)
            b2 = np.clip((128 * (saa[:, None] * sbt - sab[:, None] * sat) + dd) // (2 * dd), 0, 65535)
            e2[:, r, 0], e2[:, r, 1] = np.where(can[:, r, None], a2, e[:, r, 0]), np.where(can[:, r, None], b2, e[:, r, 1])
        idx2, err2 = fit3(e2, region, h, inside)
        better = can & (err2 < err)                              # per region
        e = np.where(better[:, :, None, None], e2, e)
        idx = np.where(np.take_along_axis(better, region, axis=1), idx2, idx)
        err = np.where(better, err2, err)
        going = better
    empty1 = ~(inside & (region == 1)).any(axis=1)
    e[:, 1] = np.where(empty1[:, None, None], e[:, 0], e[:, 1])

    # steps 5 and 6: the ten modes against the one-region result; strictly smaller replaces
    anchor = ANCHOR[shape]
    rows = np.arange(nb)
    best_err, best_mode = one_err.copy(), one_mode.copy()
    best_q, best_idx = np.zeros((nb, 2, 2, 3), np.int64), np.zeros((nb, 16), np.int64)
    for mode in TWO_REGION:
        bits, delta, transformed = bc6h_ref.MODES[mode][:3]
        q = e >> (16 - bits)
        mi, me = fit3(bc6h_ref.unquantize(q, bits), region, h, inside)
        me = me.sum(axis=1)
        flip = np.stack([mi[:, 0] >= 4, mi[rows, anchor] >= 4], axis=1)      # (an anchor outside the level has index 0)
        q = np.where(flip[:, :, None, None], q[:, :, ::-1], q)
        mi = np.where(np.take_along_axis(flip, region, axis=1) & inside, 7 - mi, mi)
        ok = np.ones(nb, bool)
        if transformed:
            half = 1 << (np.array(delta, np.int64) - 1)
            for d in (q[:, 0, 1] - q[:, 0, 0], q[:, 1, 0] - q[:, 0, 0], q[:, 1, 1] - q[:, 0, 0]):
                ok &= ((d >= -half) & (d < half)).all(axis=1)
        take = ok & (me < best_err)
        best_err, best_mode = np.where(take, me, best_err), np.where(take, mode, best_mode)
        best_q, best_idx = np.where(take[:, None, None, None], q, best_q), np.where(take[:, None], mi, best_idx)

    # step 7
    blocks = one_blocks.copy()
    for mode in TWO_REGION:
        bits, delta, transformed = bc6h_ref.MODES[mode][:3]
        sel = np.nonzero(best_mode == mode)[0]
        if not len(sel):
            continue
        bits128 = np.zeros((len(sel), 128), np.uint8)
        for k in range(2 if mode < 2 else 5):
            bits128[:, k] = (mode >> k) & 1
        q, mi = best_q[sel], best_idx[sel]
        assert (mi[:, 0] < 4).all() and (mi[np.arange(len(sel)), anchor[sel]] < 4).all()
        field = {}
        for ci, c in enumerate("rgb"):
            e0 = q[:, 0, 0, ci]
            field[c + "0"] = e0
            for i, v in ((1, q[:, 0, 1, ci]), (2, q[:, 1, 0, ci]), (3, q[:, 1, 1, ci])):
                field[c + str(i)] = (v - e0) & ((1 << delta[ci]) - 1) if transformed else v         # two's complement of the width
        for pos, name, k in bc6h_ref.header_bits(mode):
            bits128[:, pos] = (field[name] >> k) & 1
        for k in range(5):
            bits128[:, 77 + k] = (shape[sel] >> k) & 1
        pos = np.full(len(sel), 82)
        for tx in range(16):
            width = np.where((tx == 0) | (tx == anchor[sel]), 2, 3)
            for k in range(3):
                on = k < width
                bits128[np.nonzero(on)[0], pos[on] + k] = (mi[on, tx] >> k) & 1
            pos = pos + width
        assert (pos == 128).all()
        blocks[sel] = np.packbits(bits128, axis=1, bitorder="little")
    return blocks, best_err, best_mode, shape


def encode_level(rgb, chunk=512):
    """a level float32 [s, s, >= 3] -> (blocks uint8 [blocks, 16] row-major, predicted error, mode, searched shape)"""
    h, inside = enc.level_texels(rgb)
    parts = [encode_blocks(h[o:o + chunk], inside[o:o + chunk]) for o in range(0, len(h), chunk)]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4))


def encode_cube(cube, size, mip_levels):
    """the pbr_cube_f32 chain -> six face chains (uint8, bc6h_ref.chain_bytes each): what pbr_bc6h_encode_cube_ex writes with
    PBR_BC6H_ENCODE_TWO_REGION"""
    faces = [[] for _ in range(6)]
    for level in enc.cube_levels(cube, size, mip_levels):
        blocks = encode_level6(level)[0]                         # (the six faces of a level in one go: fewer, larger arrays)
        for f in range(6):
            faces[f].append(blocks[f].reshape(-1))
    return [np.concatenate(f) for f in faces]


def encode_level6(level, chunk=512):
    """the six faces of a level, float32 [6][s, s, >= 3] -> (blocks [6, n, 16], predicted error [6, n], mode [6, n], shape [6, n])"""
    parts = [enc.level_texels(level[f]) for f in range(6)]
    h, inside = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    out = [encode_blocks(h[o:o + chunk], inside[o:o + chunk]) for o in range(0, len(h), chunk)]
    return tuple(np.concatenate([p[k] for p in out]).reshape((6, -1) + out[0][k].shape[1:]) for k in range(4))
