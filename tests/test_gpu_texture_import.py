"""Texture import on the GPU (include/pbr_hip.h: pbr_texture2d_gen_mips, pbr_bc1_encode): the mip chain against scene.mip_chain and
the BC1 blocks against the numpy restatement of the pinned rule (tests/bc1_encode_ref.py), both bit for bit; the round trip through
pbr_bc1_decode; imported textures in the textured raster; refusals; the host library's import into the reference's texture file.
Reads tests/golden/ only."""
import ctypes as C

import numpy as np
import pytest
import torch

import bc1_encode_ref
import bc1_ref
from direct12pbrrenderer_amd import scene
from direct12pbrrenderer_amd.structs import TEX_BC1_BLOCKS, Tile, texture2d_bytes
from test_gpu_raster import same
from test_gpu_raster_tex import gpu_raster_tex, reference_textured_scene
from test_texture_import_cpu import FORMATS, fixture_images, gradient_noise_image, noise_image, stored_level0

pytestmark = pytest.mark.gpu
FILL = 0x5A


def random_level0(rng, w, h, fmt):
    return rng.integers(0, 256, (h, w) if fmt == 61 else (h, w, 4), dtype=np.uint8)


def chain_with_level0(ctx, lv0, mips, fmt, lead=0):
    """a device buffer filled with FILL holding a chain-sized view `lead` bytes in, with level 0 uploaded: (buffer, view)"""
    h, w = lv0.shape[:2]
    n = texture2d_bytes(w, h, mips, fmt)
    buf = ctx.empty((lead + n + 16,), torch.uint8)
    buf.fill_(FILL)
    view = buf[lead:lead + n]
    view[:lv0.size].copy_(torch.from_numpy(np.ascontiguousarray(lv0).reshape(-1)))
    return buf, view


def test_gen_mips_equals_scene_mip_chain(ctx):
    """pbr_texture2d_gen_mips == scene.mip_chain, bit for bit: the four formats; square, non-square (64 x 16), odd levels (100 x 60,
    37 x 21: rows that are not aligned to the vector loads), one-level, partial and full chains, chains above seven levels (the
    second launch), an R8 chain at an odd address; nothing is written outside the chain"""
    rng = np.random.default_rng(31)
    cases = [(64, 64, None), (64, 16, None), (100, 60, None), (100, 60, 3), (37, 21, None), (130, 70, 1), (2, 2, None), (1, 1, None),
             (256, 256, None), (512, 128, None), (200, 333, None), (1024, 1024, 9)]
    for fmt in FORMATS:
        for w, h, mips in cases:
            lv0 = random_level0(rng, w, h, fmt)
            want = scene.pack_chain(scene.mip_chain(lv0, mips)).view(np.uint8).reshape(-1)
            n_levels = min(w, h).bit_length() if mips is None else mips
            for lead in ((0, 1, 3) if fmt == 61 else (0, 4)):
                buf, view = chain_with_level0(ctx, lv0, n_levels, fmt, lead)
                ctx.texture2d_gen_mips(view, w, h, n_levels, fmt)
                ctx.sync()
                got = buf.cpu().numpy()
                assert want.size == view.numel()
                assert np.array_equal(got[lead:lead + want.size], want), (fmt, w, h, mips, lead)
                assert (got[:lead] == FILL).all() and (got[lead + want.size:] == FILL).all(), (fmt, w, h, mips, lead)


@pytest.mark.parametrize("fmt", [28, 61])
def test_gen_mips_at_a_real_size(ctx, fmt):
    """2048^2 x 12 levels of seeded bytes, the size of the scene's larger maps"""
    lv0 = random_level0(np.random.default_rng(32), 2048, 2048, fmt)
    buf, view = chain_with_level0(ctx, lv0, 12, fmt)
    ctx.texture2d_gen_mips(view, 2048, 2048, 12, fmt)
    ctx.sync()
    want = scene.pack_chain(scene.mip_chain(lv0)).view(np.uint8).reshape(-1)
    got = buf.cpu().numpy()
    assert np.array_equal(got[:want.size], want) and (got[want.size:] == FILL).all()


def encode_cases():
    """(what, stored format, the chain's levels in that format)"""
    cases = []
    for n, k, fmt, rgb in fixture_images():                  # the 20 fixture images in their own stored formats, full chains
        cases.append((f"{n} {k}", fmt, scene.mip_chain(stored_level0(rgb, fmt))))
    rng = np.random.default_rng(33)
    for fmt in FORMATS:                                      # every format on noise, gradient + noise and odd sizes
        cases.append(("noise", fmt, scene.mip_chain(random_level0(rng, 64, 32, fmt))))
        cases.append(("gradient", fmt, scene.mip_chain(stored_level0(gradient_noise_image(34, 96, 64), fmt))))
        cases.append(("odd", fmt, scene.mip_chain(random_level0(rng, 37, 21, fmt))))
        cases.append(("12 -> 6 -> 3", fmt, scene.mip_chain(stored_level0(gradient_noise_image(35, 12, 12), fmt), 3)))
        cases.append(("one level", fmt, scene.mip_chain(stored_level0(noise_image(36, 50, 19), fmt), 1)))
    # three levels of sides that are no multiple of 4, down to one block (20 -> 10 -> 5) and down to a row of two texels (9 x 5 -> 2 x 1)
    cases.append(("20 x 12 x 3", 61, scene.mip_chain(random_level0(rng, 20, 12, 61), 3)))
    cases.append(("9 x 5 x 3", 87, scene.mip_chain(random_level0(rng, 9, 5, 87), 3)))
    return cases


def test_bc1_encode_equals_the_restatement_and_decodes_to_it(ctx):
    """pbr_bc1_encode == tests/bc1_encode_ref.py, bit for bit (partial blocks included), nothing written past the blocks; and
    pbr_bc1_decode of the GPU's blocks is bc1_ref's decode of the restatement's"""
    cases = encode_cases()
    assert len(cases) == 20 + 5 * len(FORMATS) + 2 and {c[1] for c in cases[:20]} == set(FORMATS) and all(len(c[2]) == 8 for c in cases[:20])
    for what, fmt, levels in cases:
        h, w = levels[0].shape[:2]
        mips = len(levels)
        want = bc1_encode_ref.encode_chain(levels, fmt)
        assert want.size == texture2d_bytes(w, h, mips, fmt | TEX_BC1_BLOCKS)
        pair = ctx.upload_texture(scene.pack_chain(levels), w, h, mips, fmt)
        out = ctx.empty((want.size + 16,), torch.uint8)
        out.fill_(FILL)
        blocks, desc = ctx.bc1_encode(pair, w, h, mips, fmt, out=out[:want.size])
        assert (desc.width, desc.height, desc.mip_levels, desc.format) == (w, h, mips, fmt | TEX_BC1_BLOCKS)
        decoded, _ = ctx.bc1_decode(blocks, w, h, mips, fmt)
        ctx.sync()
        got = out.cpu().numpy()
        assert np.array_equal(got[:want.size], want), (what, fmt, w, h)
        assert (got[want.size:] == FILL).all(), (what, fmt)
        assert np.array_equal(decoded.cpu().numpy(), scene.pack_chain(bc1_ref.decode_chain(want, w, h, mips, fmt)).reshape(-1)), (what, fmt)
    # an R8 chain read from an odd address: the rows fall back to byte loads
    levels = scene.mip_chain(random_level0(np.random.default_rng(37), 40, 24, 61))
    packed = scene.pack_chain(levels)
    buf = ctx.empty((packed.size + 1,), torch.uint8)
    buf[1:].copy_(torch.from_numpy(packed))
    blocks, _ = ctx.bc1_encode(buf[1:], 40, 24, len(levels), 61)
    ctx.sync()
    assert np.array_equal(blocks.cpu().numpy(), bc1_encode_ref.encode_chain(levels, 61))


def test_imported_textures_in_the_raster(ctx, orc):
    """The four textured reference models with every texture brought in by import_texture(level 0): the five planes of the same
    scene with scene.mip_chain's chains through upload_texture, bit for bit.  With bc1=True: the planes of the table pbr_bc1_decode
    makes of the same blocks (the in-place contract); how far they are from the uncompressed run is printed, not asserted."""
    w, h = 1440, 960
    g, v, i, d, maps, texs, _, _, _ = reference_textured_scene(w, h, orc)
    tile = Tile(0, 0, w, h, w, h)
    assert len(texs) == 20 and {t["format"] for t in texs} == set(FORMATS)

    def raster(pairs):
        return gpu_raster_tex(ctx, g, tile, v, i, d, maps, [], descs=[p[1] for p in pairs])
    chains = [scene.mip_chain(t["levels"][0]) for t in texs]
    uploaded = [ctx.upload_texture(scene.pack_chain(c), t["width"], t["height"], len(c), t["format"]) for c, t in zip(chains, texs)]
    imported = scene.import_texture_table(ctx, texs)
    for (dev, desc), c, t in zip(imported, chains, texs):
        assert (desc.width, desc.height, desc.mip_levels, desc.format) == (t["width"], t["height"], len(c), t["format"])
        assert np.array_equal(dev.cpu().numpy(), scene.pack_chain(c).view(np.uint8).reshape(-1))
    want = raster(uploaded)
    assert (((want["C"] >> 16) & 255) > 0).sum() > 1000
    same(raster(imported), want)
    # a partial chain through import_texture
    dev, desc = ctx.import_texture(texs[0]["levels"][0], texs[0]["format"], mip_levels=3)
    assert desc.mip_levels == 3 and np.array_equal(dev.cpu().numpy(), scene.pack_chain(chains[0][:3]).view(np.uint8).reshape(-1))
    # BC1 import: blocks of the restatement, sampled in place == sampled after pbr_bc1_decode
    compressed = scene.import_texture_table(ctx, texs, bc1=True)
    for (dev, desc), c, t in zip(compressed, chains, texs):
        assert desc.format == t["format"] | TEX_BC1_BLOCKS and desc.mip_levels == len(c)
        assert np.array_equal(dev.cpu().numpy(), bc1_encode_ref.encode_chain(c, t["format"]))
    decoded = [ctx.bc1_decode(p, t["width"], t["height"], p[1].mip_levels, t["format"]) for p, t in zip(compressed, texs)]
    got = raster(compressed)
    same(got, raster(decoded))
    differing = sum(int((got[k].view(np.uint8) != want[k].view(np.uint8)).sum()) for k in ("A", "B", "C"))
    print(f"BC1 import at {w}x{h}: {differing} of {3 * 4 * w * h} A/B/C bytes differ from the uncompressed run "
          f"({100.0 * differing / (3 * 4 * w * h):.3f} %)")
    for k in ("depth", "stencil"):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8))


def test_refusals_enqueue_nothing(ctx):
    """every refusal of both entry points returns an error that names the entry point, a following pbr_sync succeeds and the
    buffers keep their fill pattern; a one-level chain is valid and changes nothing"""
    lib, hdl = ctx.lib, ctx.h
    chain = ctx.empty((texture2d_bytes(16, 8, 4, 87) + 8,), torch.uint8)
    blocks = ctx.empty((texture2d_bytes(16, 8, 4, 87 | TEX_BC1_BLOCKS) + 8,), torch.uint8)
    chain.fill_(7)
    blocks.fill_(7)
    tp, bp = chain.data_ptr(), blocks.data_ptr()
    assert tp % 8 == 0 and bp % 8 == 0
    for ptr, w, h, mips, fmt in ((0, 16, 8, 4, 87), (tp + 2, 16, 8, 4, 87), (tp + 1, 16, 8, 4, 28), (tp, 0, 8, 1, 87), (tp, 16, 0, 1, 87),
                                 (tp, 16385, 8, 1, 87), (tp, 16, 16385, 1, 61), (tp, 16, 8, 0, 87), (tp, 16, 8, 5, 87), (tp, 16, 8, 4, 29),
                                 (tp, 16, 8, 4, 0), (tp, 16, 8, 4, 87 | TEX_BC1_BLOCKS), (tp, 16, 8, 4, 87 | 0x200),
                                 (tp, 16, 8, 4, 61 | 0x80000000)):
        assert lib.pbr_texture2d_gen_mips(hdl, ptr, w, h, mips, fmt) != 0, (ptr - tp, w, h, mips, fmt)
        assert b"pbr_texture2d_gen_mips" in lib.pbr_last_error(hdl)
    for src, w, h, mips, fmt, dst in ((0, 16, 8, 4, 87, bp), (tp, 16, 8, 4, 87, 0), (tp, 16, 8, 4, 87, bp + 4), (tp, 16, 8, 4, 61, bp + 1),
                                      (tp + 2, 16, 8, 4, 87, bp), (tp, 0, 8, 1, 87, bp), (tp, 16, 16385, 1, 87, bp), (tp, 16, 8, 0, 87, bp),
                                      (tp, 16, 8, 5, 87, bp), (tp, 16, 8, 4, 29, bp), (tp, 16, 8, 4, 87 | TEX_BC1_BLOCKS, bp),
                                      (tp, 16, 8, 4, 87 | 0x10000, bp)):
        assert lib.pbr_bc1_encode(hdl, src, w, h, mips, fmt, dst) != 0, (src - tp, w, h, mips, fmt, dst - bp)
        assert b"pbr_bc1_encode" in lib.pbr_last_error(hdl)
    assert lib.pbr_texture2d_gen_mips(hdl, tp, 16, 8, 1, 87) == 0          # one level: valid, nothing to do
    ctx.sync()
    assert (chain.cpu().numpy() == 7).all() and (blocks.cpu().numpy() == 7).all()
    # valid calls still run
    ctx.texture2d_gen_mips(chain[:-8], 16, 8, 4, 87)
    ctx.bc1_encode(chain[:-8], 16, 8, 4, 87, out=blocks[:-8])
    ctx.sync()
    want = scene.mip_chain(np.full((8, 16, 4), 7, np.uint8))
    assert np.array_equal(chain.cpu().numpy()[:-8], scene.pack_chain(want).reshape(-1)) and (chain.cpu().numpy()[-8:] == 7).all()
    assert np.array_equal(blocks.cpu().numpy()[:-8], bc1_encode_ref.encode_chain(want, 87)) and (blocks.cpu().numpy()[-8:] == 7).all()


def test_host_import_writes_the_reference_file(ctx):
    """pbrh_import_texture -> pbrh_parse_texture_file: the blocks pbr_bc1_encode makes of the generated chain, in the reference's
    file layout; a level 0 whose size is no multiple of 4 is refused as the reference refuses it"""
    import struct
    from direct12pbrrenderer_amd import host
    rng = np.random.default_rng(38)
    r = host.HostRenderer(0, 256, 144, 32, 64)
    try:
        for fmt, w, h, mips in ((91, 128, 64, None), (61, 64, 64, None), (28, 256, 256, 4), (87, 12, 8, None)):
            lv0 = stored_level0(gradient_noise_image(int(rng.integers(1 << 30)), w, h), fmt)
            data = r.import_texture(lv0, fmt, mip_levels=mips)
            n_levels = min(w, h).bit_length() if mips is None else mips
            blocks, fw, fh, fm, ff = host.parse_texture_file(data)
            assert (fw, fh, fm, ff) == (w, h, n_levels, fmt | TEX_BC1_BLOCKS)
            assert data[:16] == struct.pack("<HHHHB3xI", w, h, 1, n_levels, fmt, blocks.size)
            dev, desc = ctx.import_texture(lv0, fmt, mip_levels=mips, bc1=True)
            ctx.sync()
            assert np.array_equal(blocks, dev.cpu().numpy()), (fmt, w, h)
            assert np.array_equal(blocks, bc1_encode_ref.encode_chain(scene.mip_chain(lv0, mips), fmt)), (fmt, w, h)
        for w, h in ((10, 8), (8, 6), (7, 7)):
            with pytest.raises(host.HostError, match="multiples of 4"):
                r.import_texture(np.zeros((h, w, 4), np.uint8), 28)
        with pytest.raises(host.HostError, match="bad size, level count or format"):
            r.import_texture(np.zeros((8, 8, 4), np.uint8), 28, mip_levels=5)
        err = C.create_string_buffer(256)
        lv0 = np.zeros((8, 8, 4), np.uint8)
        need = r.lib.pbrh_import_texture(r.h, None, 8, 8, 28, 4, None, 0, err, 256)
        assert need == 16 + texture2d_bytes(8, 8, 4, 28 | TEX_BC1_BLOCKS)
        out = np.full(need, 0xAB, np.uint8)
        assert r.lib.pbrh_import_texture(r.h, lv0.ctypes.data, 8, 8, 28, 4, out.ctypes.data, need - 1, err, 256) == -1
        assert b"too small" in err.value and (out == 0xAB).all()
    finally:
        r.close()
