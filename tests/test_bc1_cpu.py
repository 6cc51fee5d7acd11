"""CPU checks of BC1-resident textures (include/pbr_hip.h: PBR_TEX_BC1_BLOCKS, pbr_texture2d_bytes) through the numpy restatement
(tests/bc1_ref.py): known-answer blocks, the BC1 fixture against the decoded one, chain sizes, the texture-file reader and
upload_texture's validation."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import bc1_ref
import common
from direct12pbrrenderer_amd import _lib, scene, structs
from direct12pbrrenderer_amd.structs import (TEX_B8G8R8A8_UNORM, TEX_B8G8R8A8_UNORM_SRGB, TEX_BC1_BLOCKS, TEX_R8_UNORM,
                                             TEX_R8G8B8A8_UNORM, Texture2D)

GOLDEN = os.path.join(common.ROOT, "tests", "golden")


def block(c0, c1, indices):
    """one BC1 block from its endpoints and its 16 indices (row-major)"""
    bits = sum(int(k) << (2 * i) for i, k in enumerate(indices))
    return np.frombuffer(struct.pack("<HHI", c0, c1, bits), np.uint8)


def rgb565(r5, g6, b5):
    return (r5 << 11) | (g6 << 5) | b5


def test_known_answer_blocks():
    idx = [0, 1, 2, 3, 3, 2, 1, 0, 0, 0, 1, 1, 2, 2, 3, 3]
    # both extremes of the 565 expansion: 0 -> 0, all ones -> 255; and a middle value by replication
    assert np.array_equal(bc1_ref.palette(0xFFFF, 0x0000)[:2, :3], [[255, 255, 255], [0, 0, 0]])
    assert np.array_equal(bc1_ref.palette(rgb565(16, 32, 1), 0)[0], [132, 130, 8, 255])   # 10000 -> 10000100, 100000 -> 10000010
    # four colours (c0 > c1): white / black and the two thirds (2 * 255 + 0 + 1) // 3 = 170, (255 + 1) // 3 = 85, all opaque
    px = bc1_ref.decode_level(block(0xFFFF, 0x0000, idx), 4, 4)
    want = np.array([[255] * 3 + [255], [0] * 3 + [255], [170] * 3 + [255], [85] * 3 + [255]], np.uint8)
    assert np.array_equal(px.reshape(16, 4), want[idx])
    # three colours (c0 <= c1): the midpoint (0 + 255 + 1) // 2 = 128, and index 3 is transparent black
    px = bc1_ref.decode_level(block(0x0000, 0xFFFF, idx), 4, 4)
    want = np.array([[0] * 3 + [255], [255] * 3 + [255], [128] * 3 + [255], [0, 0, 0, 0]], np.uint8)
    assert np.array_equal(px.reshape(16, 4), want[idx])
    # equal endpoints are three-colour order: indices 0, 1, 2 the colour itself, 3 transparent black
    c = rgb565(31, 0, 9)                                                               # (255, 0, 74)
    px = bc1_ref.decode_level(block(c, c, idx), 4, 4)
    want = np.array([[255, 0, 74, 255]] * 3 + [[0, 0, 0, 0]], np.uint8)
    assert np.array_equal(px.reshape(16, 4), want[idx])
    # rounding of the thirds on uneven channels: c0 = (8, 4, 0), c1 = (0, 0, 8): (2 * 8 + 0 + 1) // 3 = 5, (8 + 1) // 3 = 3, ...
    p = bc1_ref.palette(rgb565(1, 1, 0), rgb565(0, 0, 1))
    assert np.array_equal(p[:, :3], [[8, 4, 0], [0, 0, 8], [5, 3, 3], [3, 1, 5]])
    # index bit order: texel (x, y) sits at bits 2 (4 y + x); a block whose only non-zero index is texel (2, 1)
    one = [0] * 16
    one[4 * 1 + 2] = 1
    px = bc1_ref.decode_level(block(0xFFFF, 0x0000, one), 4, 4)
    assert px[1, 2, 0] == 0 and (np.delete(px[..., 0].reshape(-1), 6) == 255).all()
    # a level smaller than a block keeps the block's top-left texels; stored orders of the four formats
    rgba = bc1_ref.decode_level(block(rgb565(31, 0, 0), rgb565(0, 0, 31), list(range(4)) * 4), 2, 1)
    assert np.array_equal(rgba, [[[255, 0, 0, 255], [0, 0, 255, 255]]])
    assert np.array_equal(bc1_ref.stored(rgba, 28), rgba) and np.array_equal(bc1_ref.stored(rgba, 61), [[255, 0]])
    for f in (87, 91):
        assert np.array_equal(bc1_ref.stored(rgba, f), [[[0, 0, 255, 255], [255, 0, 0, 255]]])


def test_fixture_blocks_decode_to_the_decoded_fixture():
    """the BC1 fixture's 32 x 32 level and below, decoded by bc1_ref into the stored format, are textured_models.npz's texels,
    byte for byte, for all 20 maps; both block orders occur in the kept data"""
    fxb = np.load(os.path.join(GOLDEN, "textured_models_bc1.npz"))
    fxt = np.load(os.path.join(GOLDEN, "textured_models.npz"))
    assert os.path.getsize(os.path.join(GOLDEN, "textured_models_bc1.npz")) < os.path.getsize(os.path.join(GOLDEN, "textured_models.npz"))
    assert [str(n) for n in fxb["name"]] == [str(n) for n in fxt["name"]] and list(fxb["maps"]) == list(fxt["maps"])
    table = scene.bc1_texture_table(fxb)
    decoded, _ = scene.add_textured_models(scene.MeshScene(), fxt)
    assert len(table) == len(decoded) == 20
    n_maps, formats, three, blocks = 0, set(), 0, 0
    for n in fxb["name"]:
        for k in fxb["maps"]:
            if f"{n}_{k}_blocks" not in fxb.files:
                assert f"{n}_{k}_texels" not in fxt.files
                continue
            w0, h0, mips0, fmt, w, h, mips = (int(x) for x in fxb[f"{n}_{k}_info"])
            assert (w, h) == (128, 128) and mips == 8 and (w0 >> (mips0 - mips), h0 >> (mips0 - mips)) == (w, h)
            assert tuple(fxt[f"{n}_{k}_info"][:4]) == (w0, h0, mips0, fmt) and tuple(fxt[f"{n}_{k}_info"][4:]) == (32, 32, 6)
            t, d = table[n_maps], decoded[n_maps]
            assert (t["width"], t["height"], t["mips"], t["format"]) == (w, h, mips, fmt) and d["format"] == fmt
            levels = bc1_ref.decode_chain(t["blocks"], w, h, mips, fmt)
            assert np.array_equal(scene.pack_chain(levels[2:]), fxt[f"{n}_{k}_texels"]), (n, k)
            b = np.asarray(t["blocks"]).reshape(-1, 8).astype(np.int64)
            three += int(((b[:, 0] + 256 * b[:, 1]) <= (b[:, 2] + 256 * b[:, 3])).sum())
            blocks += len(b)
            formats.add(fmt)
            n_maps += 1
    assert n_maps == 20 and formats == {28, 87, 91, 61}
    assert 0.1 < three / blocks < 0.5, three / blocks            # both modes are exercised by real data


def test_chain_sizes():
    lib = _lib.load()
    # the reference's asset files minus their 16-byte header
    for w, mips, want in ((1024, 11, 699064), (2048, 12, 2796216)):
        for fmt in (28, 87, 91, 61):
            assert lib.pbr_texture2d_bytes(w, w, mips, fmt | TEX_BC1_BLOCKS) == want
            assert structs.texture2d_bytes(w, w, mips, fmt | TEX_BC1_BLOCKS) == want == bc1_ref.chain_bytes(w, w, mips, fmt | 0x100)
    # the three statements agree, decoded chains with pack_chain, on odd shapes and partial chains
    rng = np.random.default_rng(3)
    for w, h, mips in ((1, 1, 1), (4, 4, 3), (5, 3, 2), (13, 7, 3), (37, 21, 5), (128, 32, 4), (19, 50, 5), (16384, 16384, 15)):
        for fmt in (TEX_R8G8B8A8_UNORM, TEX_B8G8R8A8_UNORM, TEX_B8G8R8A8_UNORM_SRGB, TEX_R8_UNORM):
            got = lib.pbr_texture2d_bytes(w, h, mips, fmt)
            assert got == structs.texture2d_bytes(w, h, mips, fmt) == bc1_ref.chain_bytes(w, h, mips, fmt) > 0
            if w <= 256:
                ch = 1 if fmt == TEX_R8_UNORM else 4
                lv0 = rng.integers(0, 256, (h, w, ch) if ch == 4 else (h, w), dtype=np.uint8)
                assert got == scene.pack_chain(scene.mip_chain(lv0, mips)).size
            b = lib.pbr_texture2d_bytes(w, h, mips, fmt | TEX_BC1_BLOCKS)
            assert b == structs.texture2d_bytes(w, h, mips, fmt | TEX_BC1_BLOCKS) == bc1_ref.chain_bytes(w, h, mips, fmt | 0x100)
            assert b == sum(8 * max(1, ((w >> l) + 3) // 4) * max(1, ((h >> l) + 3) // 4) for l in range(mips))
    # invalid descriptions: 0 from all three
    for w, h, mips, fmt in ((0, 4, 1, 28), (4, 0, 1, 28), (16385, 4, 1, 28), (4, 4, 0, 28), (4, 4, 4, 28), (5, 3, 3, 61), (4, 4, 1, 29),
                            (4, 4, 1, 0x100), (4, 4, 1, 28 | 0x200), (4, 4, 1, 28 | 0x100 | 0x1000), (4, 4, 1, 0x100 | 29)):
        assert lib.pbr_texture2d_bytes(w, h, mips, fmt) == 0, (w, h, mips, fmt)
        assert structs.texture2d_bytes(w, h, mips, fmt) == 0 and bc1_ref.chain_bytes(w, h, mips, fmt) == 0, (w, h, mips, fmt)


def texture_file(blocks, w, h, mips, fmt, depth=1, count=None):
    blocks = np.asarray(blocks, np.uint8)
    return struct.pack("<HHHHB3xI", w, h, depth, mips, fmt, blocks.size if count is None else count) + blocks.tobytes()


def test_texture_file_reader():
    """a file in the reference's layout, written here from fixture blocks, round-trips through pbrh_parse_texture_file; every
    refusal names its reason and writes nothing"""
    import torch  # noqa: F401  (its ROCm runtime first: see _lib.load)
    from direct12pbrrenderer_amd import host
    L = C.CDLL(common.host_lib_path())
    L.pbrh_parse_texture_file.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    fxb = np.load(os.path.join(GOLDEN, "textured_models_bc1.npz"))
    err = C.create_string_buffer(256)
    for t in scene.bc1_texture_table(fxb)[::3]:
        data = texture_file(t["blocks"], t["width"], t["height"], t["mips"], t["format"])
        assert data[:12] == struct.pack("<HHHHB3x", 128, 128, 1, 8, t["format"]) and len(data) == 16 + t["blocks"].size
        desc, out = Texture2D(), np.full(t["blocks"].size + 8, 0xAB, np.uint8)
        assert L.pbrh_parse_texture_file(data, len(data), C.addressof(desc), out.ctypes.data, out.size, err, 256) == 0, err.value
        assert (desc.width, desc.height, desc.mip_levels, desc.format) == (128, 128, 8, t["format"] | TEX_BC1_BLOCKS)
        assert desc.texels == out.ctypes.data
        assert np.array_equal(out[:-8], t["blocks"]) and (out[-8:] == 0xAB).all()
        # the description alone
        assert L.pbrh_parse_texture_file(data, len(data), C.addressof(desc), None, 0, err, 256) == 0 and not desc.texels
        # the Python binding
        blocks, w, h, mips, fmt = host.parse_texture_file(data)
        assert np.array_equal(blocks, t["blocks"]) and (w, h, mips, fmt) == (128, 128, 8, t["format"] | TEX_BC1_BLOCKS)
    # a non-square chain with levels smaller than a block
    blk = np.arange(bc1_ref.chain_bytes(13, 7, 3, 61 | 0x100), dtype=np.uint8)
    assert host.parse_texture_file(texture_file(blk, 13, 7, 3, 61))[1:] == (13, 7, 3, 61 | TEX_BC1_BLOCKS)
    t = scene.bc1_texture_table(fxb)[0]
    good = texture_file(t["blocks"], 128, 128, 8, t["format"])
    n = t["blocks"].size
    refusals = [(good[:9], b"truncated"), (good[:15], b"truncated"), (good[:-1], b"truncated"), (good[:16], b"truncated"),
                (good + b"\0", b"after the payload"),
                (texture_file(t["blocks"], 128, 128, 8, t["format"], count=n - 8), b"payload"),
                (texture_file(t["blocks"], 128, 128, 8, t["format"], count=n + 8), b"payload"),
                (texture_file(t["blocks"], 128, 128, 7, t["format"]), b"payload"),
                (texture_file(t["blocks"], 128, 128, 8, t["format"], depth=2), b"depth"),
                (texture_file(t["blocks"], 128, 128, 8, t["format"], depth=0), b"depth"),
                (texture_file(t["blocks"], 128, 128, 8, 71), b"format"), (texture_file(t["blocks"], 128, 128, 8, 0), b"format"),
                (texture_file(t["blocks"], 128, 128, 9, t["format"]), b"level count"),
                (texture_file(t["blocks"], 0, 128, 8, t["format"]), b"size")]
    for data, why in refusals:
        desc, out = Texture2D(0x55, 1, 2, 3, 4), np.full(n, 0xAB, np.uint8)
        err.value = b""
        assert L.pbrh_parse_texture_file(data, len(data), C.addressof(desc), out.ctypes.data, out.size, err, 256) == -1, why
        assert why in err.value, (why, err.value)
        assert (desc.texels, desc.width, desc.height, desc.mip_levels, desc.format) == (0x55, 1, 2, 3, 4) and (out == 0xAB).all(), why
        with pytest.raises(host.HostError):
            host.parse_texture_file(data)
    # an output buffer that is too small
    desc, out = Texture2D(0x55, 1, 2, 3, 4), np.full(n - 1, 0xAB, np.uint8)
    assert L.pbrh_parse_texture_file(good, len(good), C.addressof(desc), out.ctypes.data, out.size, err, 256) == -1
    assert b"too small" in err.value and desc.width == 1 and (out == 0xAB).all()


def test_upload_texture_validates_bc1_chains_before_the_device():
    """upload_texture's checks of a BC1 chain raise before anything touches a device (none is needed for them)"""
    from direct12pbrrenderer_amd.api import PbrContext, PbrError
    ctx = PbrContext.__new__(PbrContext)           # no device: the refusals below come first
    blocks = np.zeros(structs.texture2d_bytes(16, 8, 4, 28 | TEX_BC1_BLOCKS), np.uint8)
    assert blocks.size == 8 * (4 * 2 + 2 + 1 + 1)
    for chain, w, h, mips, fmt, why in ((blocks[:-8], 16, 8, 4, 28 | TEX_BC1_BLOCKS, "bytes"), (blocks, 16, 8, 3, 28 | TEX_BC1_BLOCKS, "bytes"),
                                        (np.zeros(16 * 8 * 4, np.uint8), 16, 8, 1, 28 | TEX_BC1_BLOCKS, "bytes"),
                                        (blocks, 16, 8, 5, 28 | TEX_BC1_BLOCKS, "bad BC1"), (blocks, 16, 8, 4, 29 | TEX_BC1_BLOCKS, "bad BC1"),
                                        (blocks, 16, 8, 4, TEX_BC1_BLOCKS, "bad BC1"), (blocks, 16, 8, 4, 28 | TEX_BC1_BLOCKS | 0x200, "bad BC1"),
                                        (blocks, 0, 8, 1, 61 | TEX_BC1_BLOCKS, "bad BC1"), (blocks, 16, 8, 4, 29, "unknown texture format"),
                                        (blocks, 16, 8, 4, 28 | 0x200, "unknown texture format")):
        with pytest.raises(PbrError, match=why):
            ctx.upload_texture(chain, w, h, mips, fmt)
    with pytest.raises(PbrError, match="bad texture description"):
        ctx.bc1_decode(None, 16, 8, 4, 28 | TEX_BC1_BLOCKS)
    with pytest.raises(PbrError, match="bad texture description"):
        ctx.bc1_decode(None, 16, 8, 5, 28)
    ctx.h = None                                   # (nothing to destroy)
