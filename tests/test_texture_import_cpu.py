"""CPU checks of the texture import path (include/pbr_hip.h: pbr_texture2d_gen_mips, pbr_bc1_encode): the numpy restatement of the
encoding rule (tests/bc1_encode_ref.py) against a third-party encoder's blocks (tests/golden/bc1_encode_yardstick.npz, written by
Pillow at fixture time; never imported here), the properties of the rule that need no yardstick, the texture-file writer against
the reader, and the binding's size checks.  The GPU is held to the restatement bit for bit in tests/test_gpu_texture_import.py."""
import ctypes as C
import os

import numpy as np
import pytest

import bc1_encode_ref
import bc1_ref
import common
from direct12pbrrenderer_amd import _lib, scene, structs
from direct12pbrrenderer_amd.structs import TEX_BC1_BLOCKS, Texture2D

GOLDEN = os.path.join(common.ROOT, "tests", "golden")
FORMATS = (28, 87, 91, 61)


def fixture_images():
    """(model, map, stored format, level 0 of the chain as [128, 128, 3] R, G, B) for the 20 chains of the BC1 fixture, decoded
    by bc1_ref; read as R, G, B whatever the chain's stored format (as the yardstick was taken)"""
    fxb = np.load(os.path.join(GOLDEN, "textured_models_bc1.npz"))
    for n in (str(x) for x in fxb["name"]):
        for k in (str(x) for x in fxb["maps"]):
            if f"{n}_{k}_blocks" not in fxb.files:
                continue
            _, _, _, fmt, w, h, _ = (int(x) for x in fxb[f"{n}_{k}_info"])
            bw, bh = bc1_ref.level_blocks(w, h)
            yield n, k, fmt, np.ascontiguousarray(bc1_ref.decode_level(fxb[f"{n}_{k}_blocks"][:8 * bw * bh], w, h)[..., :3])


def stored_level0(rgb, fmt):
    """an R, G, B image as level 0 in the stored format (alpha 255; R8 keeps red)"""
    rgba = np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=-1)
    return np.ascontiguousarray(bc1_ref.stored(rgba, fmt))


def noise_image(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def gradient_noise_image(seed, w, h):
    """three different ramps (one falling, so channels correlate negatively) plus a little noise"""
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([255 * x / max(w - 1, 1), 255 - 255 * y / max(h - 1, 1), 255 * (x + y) / max(w + h - 2, 1)], axis=-1)
    return np.clip(base + np.random.default_rng(seed).integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)


def split(blocks):
    """blocks -> (c0, c1, indices [blocks, 16]) as int64"""
    b = np.asarray(blocks, np.uint8).reshape(-1, 8).astype(np.int64)
    bits = b[:, 4] | (b[:, 5] << 8) | (b[:, 6] << 16) | (b[:, 7] << 24)
    return b[:, 0] | (b[:, 1] << 8), b[:, 2] | (b[:, 3] << 8), (bits[:, None] >> (2 * np.arange(16))) & 3


def test_new_symbols_are_exported():
    lib = _lib.load()
    assert lib.pbr_texture2d_gen_mips and lib.pbr_bc1_encode
    assert {"pbr_texture2d_gen_mips", "pbr_bc1_encode"} <= set(_lib.SIGNATURES)


def test_restatement_against_the_yardstick():
    """Quality under the pinned decode against Pillow's blocks.  Per level-0 image (decodes of real BC1 blocks): total squared error
    <= Pillow's, all 20.  Levels 1 - 3 (box-filtered, not BC1-representable): the squared error summed over the 60 levels <=
    Pillow's sum; per level it is printed, not asserted."""
    y = np.load(os.path.join(GOLDEN, "bc1_encode_yardstick.npz"))
    assert int(y["levels"]) == 4
    n_images, own0, pil0, own_low, pil_low, worse, exact, blocks = 0, 0, 0, 0, 0, [], 0, 0
    for n, k, _, rgb in fixture_images():
        for l, img in enumerate(scene.mip_chain(rgb, 4)):
            mine = bc1_encode_ref.encode_rgb(img)
            theirs = y[f"{n}_{k}_l{l}"]
            assert mine.size == theirs.size == 8 * (img.shape[0] // 4) * (img.shape[1] // 4)
            e_own, e_pil = bc1_encode_ref.squared_error(mine, img), bc1_encode_ref.squared_error(theirs, img)
            print(f"{n} {k} level {l}: squared error {e_own} (Pillow {e_pil})")
            if l == 0:
                assert e_own <= e_pil, (n, k, e_own, e_pil)
                own0, pil0 = own0 + e_own, pil0 + e_pil
                d = bc1_ref.decode_level(mine, 128, 128)[..., :3] != img
                exact += int((~d.reshape(32, 4, 32, 4, 3).any(axis=(1, 3, 4))).sum())
                blocks += 32 * 32
            else:
                own_low, pil_low = own_low + e_own, pil_low + e_pil
                if e_own > e_pil:
                    worse.append((n, k, l))
        n_images += 1
    print(f"level 0: summed squared error {own0} (Pillow {pil0}), {exact} of {blocks} blocks reproduced exactly; "
          f"levels 1-3: {own_low} (Pillow {pil_low}), worse than Pillow on {worse}")
    assert n_images == 20
    assert own_low <= pil_low, (own_low, pil_low)


def check_block_properties(rgb, blocks, what):
    """c0 >= c1; equal endpoints carry index 0 only (so the three-colour mode's index 3 never occurs); otherwise every texel of the
    level has the nearest entry of the pinned palette, the lowest index on ties; texels outside the level have index 0"""
    x, m = bc1_encode_ref.blocks_of(np.asarray(rgb).astype(np.int64))
    c0, c1, idx = split(blocks)
    assert len(c0) == len(x), what
    assert (c0 >= c1).all(), what
    assert (idx[c0 == c1] == 0).all(), what
    assert (idx[~m] == 0).all(), what
    pal = bc1_ref.palette(c0, c1)
    four = c0 > c1
    assert (pal[four][..., 3] == 255).all()
    d = ((x[:, :, None, :] - pal[:, None, :, :3]) ** 2).sum(-1)
    nearest = d.argmin(-1)
    assert np.array_equal(idx[four][m[four]], nearest[four][m[four]]), what


def test_block_properties():
    cases = [("noise", noise_image(1, 64, 48)), ("gradient", gradient_noise_image(2, 96, 64)), ("odd", noise_image(3, 37, 21)),
             ("flat", np.full((8, 8, 3), 77, np.uint8)), ("tiny", gradient_noise_image(4, 2, 2))]
    cases += [(f"{n} {k}", rgb) for n, k, _, rgb in list(fixture_images())[::4]]
    for what, rgb in cases:
        blocks = bc1_encode_ref.encode_rgb(rgb)
        check_block_properties(rgb, blocks, what)
        # the stored formats say the same thing: 28 and the swizzled 87 / 91 give the blocks of the R, G, B image, 61 those of (r, r, r)
        for fmt in FORMATS:
            want = bc1_encode_ref.encode_rgb(np.repeat(rgb[..., :1], 3, axis=-1)) if fmt == 61 else blocks
            assert np.array_equal(bc1_encode_ref.encode_level(stored_level0(rgb, fmt), fmt), want), (what, fmt)
    flat = split(bc1_encode_ref.encode_rgb(np.full((4, 4, 3), 255, np.uint8)))
    assert flat[0][0] == flat[1][0] == 0xFFFF and (flat[2] == 0).all()


def test_two_representable_colours_round_trip():
    """a block of at most two distinct colours that RGB565 holds exactly decodes to itself"""
    rng = np.random.default_rng(5)
    n = 400
    ends = bc1_ref.palette(rng.integers(0, 65536, n), rng.integers(0, 65536, n))[:, :2, :3]         # [n, 2 colours, 3]
    ends[::7, 1] = ends[::7, 0]                                                                     # some blocks of one colour
    pick = rng.integers(0, 2, (n, 16))
    x = np.take_along_axis(ends, pick[..., None].repeat(3, -1), 1)                                  # [n, 16, 3]
    img = x.reshape(n, 4, 4, 3).transpose(1, 0, 2, 3).reshape(4, 4 * n, 3).astype(np.uint8)
    blocks = bc1_encode_ref.encode_rgb(img)
    out = bc1_ref.decode_level(blocks, 4 * n, 4)
    assert np.array_equal(out[..., :3], img) and (out[..., 3] == 255).all()
    check_block_properties(img, blocks, "two colours")


def test_partial_blocks_ignore_outside_texels():
    """levels smaller than a block (2 x 2, 1 x 1) and levels whose size is no multiple of 4 (the chain 12 x 12 -> 6 x 6 -> 3 x 3):
    whatever the texels outside the level hold changes no output bit; they get index 0"""
    rng = np.random.default_rng(6)
    levels = scene.mip_chain(gradient_noise_image(7, 12, 12))[:3] + [noise_image(8, 2, 2), noise_image(9, 1, 1), noise_image(10, 5, 7)]
    assert [lv.shape[:2] for lv in levels[:3]] == [(12, 12), (6, 6), (3, 3)]
    for lv in levels:
        h, w, _ = lv.shape
        bw, bh = bc1_ref.level_blocks(w, h)
        want = bc1_encode_ref.encode_rgb(lv)
        assert want.size == 8 * bw * bh
        for outside in (255, rng.integers(0, 256, (4 * bh, 4 * bw, 3)), rng.integers(0, 256, (4 * bh, 4 * bw, 3))):
            assert np.array_equal(bc1_encode_ref.encode_rgb(lv, outside=outside), want), (w, h)
        check_block_properties(lv, want, (w, h))
        # and the decode of the level's texels is as close as the same texels in a full block would get with those indices
        assert np.array_equal(bc1_ref.decode_level(want, w, h)[..., 3], np.full((h, w), 255))
    # a 1 x 1 level is its colour quantised: both endpoints equal
    c0, c1, idx = split(bc1_encode_ref.encode_rgb(levels[4]))
    assert c0[0] == c1[0] == bc1_encode_ref.quantise(levels[4].astype(np.int64))[0, 0] and (idx == 0).all()


def test_texture_file_writer_inverts_the_reader():
    """pbrh_write_texture_file o pbrh_parse_texture_file is the identity on the 20 fixture chains; its refusals name their reason
    and write nothing"""
    import struct
    import torch  # noqa: F401  (its ROCm runtime first: see _lib.load)
    from direct12pbrrenderer_amd import host
    L = C.CDLL(common.host_lib_path())
    L.pbrh_write_texture_file.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.pbrh_write_texture_file.restype = C.c_long
    table = scene.bc1_texture_table(np.load(os.path.join(GOLDEN, "textured_models_bc1.npz")))
    assert len(table) == 20
    err = C.create_string_buffer(256)
    for t in table:
        blocks = np.ascontiguousarray(t["blocks"])
        fmt = t["format"] | TEX_BC1_BLOCKS
        data = host.write_texture_file(blocks, t["width"], t["height"], t["mips"], fmt)
        assert data == struct.pack("<HHHHB3xI", t["width"], t["height"], 1, t["mips"], t["format"], blocks.size) + blocks.tobytes()
        got = host.parse_texture_file(data)
        assert np.array_equal(got[0], blocks) and got[1:] == (t["width"], t["height"], t["mips"], fmt)
        # the C entry point: the size alone, then an exact and a larger buffer (the tail stays)
        desc = Texture2D(blocks.ctypes.data, t["width"], t["height"], t["mips"], fmt)
        assert L.pbrh_write_texture_file(C.addressof(desc), None, 0, err, 256) == len(data)
        out = np.full(len(data) + 8, 0xAB, np.uint8)
        assert L.pbrh_write_texture_file(C.addressof(desc), out.ctypes.data, out.size, err, 256) == len(data), err.value
        assert out[:-8].tobytes() == data and (out[-8:] == 0xAB).all()
    # a non-square chain with levels smaller than a block
    blk = np.arange(bc1_ref.chain_bytes(13, 7, 3, 61 | 0x100), dtype=np.uint8)
    assert host.parse_texture_file(host.write_texture_file(blk, 13, 7, 3, 61 | TEX_BC1_BLOCKS))[1:] == (13, 7, 3, 61 | TEX_BC1_BLOCKS)
    t = table[0]
    blocks = np.ascontiguousarray(t["blocks"])
    n = 16 + blocks.size

    def desc(**kw):
        f = dict(texels=blocks.ctypes.data, width=128, height=128, mip_levels=8, format=t["format"] | TEX_BC1_BLOCKS)
        f.update(kw)
        return Texture2D(f["texels"], f["width"], f["height"], f["mip_levels"], f["format"])
    refusals = [(desc(format=t["format"]), n, b"PBR_TEX_BC1_BLOCKS"), (desc(format=29 | TEX_BC1_BLOCKS), n, b"format"),
                (desc(format=t["format"] | TEX_BC1_BLOCKS | 0x200), n, b"format"), (desc(width=0), n, b"size"),
                (desc(height=16385), n, b"size"), (desc(mip_levels=0), n, b"level count"), (desc(mip_levels=9), n, b"level count"),
                (desc(texels=0), n, b"null blocks"), (desc(), n - 1, b"too small"), (desc(), 15, b"too small")]
    for d, size, why in refusals:
        out = np.full(n, 0xAB, np.uint8)
        err.value = b""
        assert L.pbrh_write_texture_file(C.addressof(d), out.ctypes.data, size, err, 256) == -1, why
        assert why in err.value, (why, err.value)
        assert (out == 0xAB).all(), why
    assert L.pbrh_write_texture_file(None, None, 0, err, 256) == -1 and b"null descriptor" in err.value
    with pytest.raises(host.HostError):
        host.write_texture_file(blocks, 128, 128, 8, t["format"])
    with pytest.raises(host.HostError, match="block bytes"):
        host.write_texture_file(blocks[:-8], 128, 128, 8, t["format"] | TEX_BC1_BLOCKS)


def test_binding_checks_sizes_before_the_device():
    """texture2d_gen_mips, bc1_encode and import_texture refuse a bad description or a tensor of the wrong size before anything
    touches a device (none is needed for these)"""
    import torch
    from direct12pbrrenderer_amd.api import PbrContext, PbrError
    ctx = PbrContext.__new__(PbrContext)           # no device: the refusals below come first
    chain = torch.zeros(structs.texture2d_bytes(16, 8, 4, 28), dtype=torch.uint8)
    for w, h, mips, fmt in ((16, 8, 5, 28), (16, 8, 0, 28), (0, 8, 1, 28), (16, 16385, 1, 61), (16, 8, 4, 29), (16, 8, 4, 28 | TEX_BC1_BLOCKS),
                            (16, 8, 4, 28 | 0x200)):
        with pytest.raises(PbrError, match="bad texture description"):
            ctx.texture2d_gen_mips(chain, w, h, mips, fmt)
        with pytest.raises(PbrError, match="bad texture description"):
            ctx.bc1_encode(chain, w, h, mips, fmt)
    with pytest.raises(PbrError, match="size does not match"):
        ctx.texture2d_gen_mips(chain[:-4], 16, 8, 4, 28)
    with pytest.raises(PbrError, match="size does not match"):
        ctx.texture2d_gen_mips(chain, 16, 8, 4, 61)
    with pytest.raises(PbrError, match="texel tensor's size"):
        ctx.bc1_encode(chain, 16, 8, 3, 28)
    with pytest.raises(PbrError, match="output tensor's size"):
        ctx.bc1_encode(chain, 16, 8, 4, 28, out=torch.zeros(8, dtype=torch.uint8))
    for level0, fmt, mips, why in ((np.zeros((8, 16, 4), np.uint8), 29, None, "unknown texture format"),
                                   (np.zeros((8, 16, 4), np.uint8), 28 | TEX_BC1_BLOCKS, None, "unknown texture format"),
                                   (np.zeros((8, 16), np.uint8), 28, None, "level 0 of format"),
                                   (np.zeros((8, 16, 3), np.uint8), 87, None, "level 0 of format"),
                                   (np.zeros((8, 16, 4), np.uint8), 61, None, "level 0 of format"),
                                   (np.zeros((8, 16, 4), np.uint8), 91, 5, "bad texture description"),
                                   (np.zeros((8, 16), np.uint8), 61, 0, "bad texture description")):
        with pytest.raises(PbrError, match=why):
            ctx.import_texture(level0, fmt, mip_levels=mips)
    ctx.h = None                                   # (nothing to destroy)
