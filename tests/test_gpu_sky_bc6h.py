"""The sky resident as BC6H_UF16 blocks on the GPU (include/pbr_hip.h: pbr_skybox_bc6h): the in-place resolve against pbr_skybox on the
cube pbr_bc6h_decode_cube makes of the same chains, bit for bit — random blocks at every size and LOD regime of
tests/sky_bc6h_cases.py, the fixture files sampled where they lie, the refusals, and the resident sky through DeferredFrame,
MultiViewFrame and the host graph.  Reads tests/golden/ only."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import common
import sky_bc6h_cases as cases
from direct12pbrrenderer_amd import host, synth
from direct12pbrrenderer_amd.structs import CubeBc6h, Global, Tile, bc6h_chain_bytes, cube_texels
from test_host_graph import to_half

pytestmark = pytest.mark.gpu
SENTINEL = 0x7A5C            # the half every target pixel holds before a resolve
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(HERE, "golden", "sky_bc6h.npz"), allow_pickle=False))


def target(ctx, h, w):
    t = ctx.empty((h, w, 4), torch.int16)
    t.fill_(SENTINEL)
    return t.view(torch.float16)


def resolve_both(ctx, faces, size, mips, g, tile, stencil):
    """(pbr_skybox_bc6h's target, pbr_skybox's on the decoded cube) as uint16 [h, w, 4]"""
    sten = ctx.upload(stencil)
    got, want = target(ctx, tile.h, tile.w), target(ctx, tile.h, tile.w)
    ctx.skybox_bc6h(g, tile, faces, size, mips, sten, tile.w, got, tile.w)
    cube = ctx.bc6h_decode_cube(faces, size, mips)
    ctx.skybox(g, tile, cube, size, mips, sten, tile.w, want, tile.w)
    ctx.sync()
    return to_half(got).view(np.uint16), to_half(want).view(np.uint16)


def test_bit_identity_on_random_blocks(ctx):
    """every case of sky_bc6h_cases.CASES — seeded random blocks (every mode, partition and reserved code) in cubes of 4^2 x 3, 8^2 x 4,
    12^2 x 4, 20^2 x 3 and 64^2 x 7, the six faces at unrelated device addresses, fifteen cameras, frames from 2 x 2 to 96 x 64 and the
    ragged 200 x 37 tile of 640 x 360: the uint16 view of the HDR target equals pbr_skybox's on the decoded cube, and pixels under a
    non-zero stencil keep the sentinel.  The conditions on the inputs (six faces, every level of the 8 and 12 chains as the lower level,
    fractional LODs and LOD 0, single-block and four-block footprints) are asserted here on what runs."""
    cases.assert_coverage(cases.coverage())
    dev = {}
    for size, mips in cases.CUBES:
        spacers = [ctx.empty((4096 * (f + 1) + 16,), torch.uint8) for f in range(6)]      # keep the six allocations apart
        dev[(size, mips)] = [ctx.upload(f) for f in cases.random_faces(size, mips)]
        assert len({d.data_ptr() for d in dev[(size, mips)]}) == 6 and all(d.data_ptr() % 16 == 0 for d in dev[(size, mips)])
        del spacers
    sky_pixels = differing = 0
    for case in cases.CASES:
        size, mips, g, tile, stencil = cases.case_inputs(case)
        got, want = resolve_both(ctx, dev[(size, mips)], size, mips, g, tile, stencil)
        off = stencil == 0
        assert (got[~off] == SENTINEL).all() and (want[~off] == SENTINEL).all(), case
        assert (got[off][:, 3] == 0x3C00).all(), case
        assert np.array_equal(got, want), (case, int((got != want).any(axis=-1).sum()), int(off.sum()))
        sky_pixels += int(off.sum())
        differing += len(np.unique(got[off][:, :3], axis=0))
    assert sky_pixels > 50000 and differing > 5000           # the targets did hold sky, and not one colour


def test_fixture_files_sampled_where_they_lie(ctx, fixture):
    """smooth_file and random_file of tests/golden/sky_bc6h.npz uploaded as they are and sampled at parse_cubemap_file's offsets, also
    with the file 16 and 48 bytes into its allocation: the same identity, under two cameras and a minifying frame"""
    for name in ("smooth_file", "random_file"):
        data = fixture[name]
        size, mips, offsets, _ = host.parse_cubemap_file(data.tobytes())
        for lead in (0, 16, 48):
            buf = ctx.empty((lead + data.size,), torch.uint8)
            buf[lead:].copy_(torch.from_numpy(data.copy()))
            faces = [buf.data_ptr() + lead + o for o in offsets]
            for cam, frame in (("pitch_roll", (96, 64)), ("wide_d", (8, 6)), ("up", (48, 32))):
                _, _, g, tile, stencil = cases.case_inputs(((size, mips), cam, frame + (None, 0, 0)))
                got, want = resolve_both(ctx, faces, size, mips, g, tile, stencil)
                assert np.array_equal(got, want) and (got[stencil != 0] == SENTINEL).all(), (name, lead, cam)
                assert len(np.unique(got[stencil == 0][:, :3], axis=0)) > 10, (name, lead, cam)


def test_refusals_enqueue_nothing(ctx):
    """every refusal of pbr_skybox_bc6h returns PBR_ERR_INVALID and leaves the target's fill"""
    size, mips, W, H = 8, 4, 32, 16
    n = bc6h_chain_bytes(size, mips)
    rng = np.random.default_rng(5)
    dev = [ctx.upload(rng.integers(0, 256, n + 16, dtype=np.uint8)) for _ in range(6)]
    good = [d.data_ptr() for d in dev]
    _, _, g, tile, _ = cases.case_inputs(((size, mips), "pitch_roll", (W, H, None, 0, 0)))
    sten = ctx.zeros((H, W), torch.uint8)
    out = target(ctx, H, W)
    lib = ctx.lib

    def call(faces, s, m, pitch=W, hdr_pitch=W, stencil=sten.data_ptr(), hdr=out.data_ptr(), t=tile, gg=g):
        cube = CubeBc6h((C.c_void_p * 6)(*faces), s, m) if faces is not None else None
        return lib.pbr_skybox_bc6h(ctx.h, C.byref(gg) if gg is not None else None, C.byref(t) if t is not None else None,
                                   C.byref(cube) if cube is not None else None, C.c_void_p(stencil) if stencil else None, pitch,
                                   C.c_void_p(hdr) if hdr else None, hdr_pitch)

    cases_ = {
        "null struct": dict(faces=None, s=size, m=mips),
        "null face": dict(faces=good[:3] + [None] + good[4:], s=size, m=mips),
        "a face at +8 bytes": dict(faces=good[:5] + [good[5] + 8], s=size, m=mips),
        "size 0": dict(faces=good, s=0, m=1),
        "size 6": dict(faces=good, s=6, m=1),
        "size above the maximum": dict(faces=good, s=8196, m=1),
        "mips 0": dict(faces=good, s=size, m=0),
        "mips too many": dict(faces=good, s=size, m=5),
        "pitch < w": dict(faces=good, s=size, m=mips, pitch=W - 1),
        "hdr pitch < w": dict(faces=good, s=size, m=mips, hdr_pitch=W - 1),
        "null stencil": dict(faces=good, s=size, m=mips, stencil=0),
        "null target": dict(faces=good, s=size, m=mips, hdr=0),
        "null tile": dict(faces=good, s=size, m=mips, t=None),
        "null global": dict(faces=good, s=size, m=mips, gg=None),
        "empty tile": dict(faces=good, s=size, m=mips, t=Tile(0, 0, 0, H, W, H)),
    }
    for why, kw in cases_.items():
        assert call(**kw) == -1, why
        assert lib.pbr_last_error(ctx.h), why
    ctx.sync()
    assert (to_half(out).view(np.uint16) == SENTINEL).all()
    assert call(good, size, mips) == 0                                               # and the good call does run
    ctx.sync()
    assert not (to_half(out).view(np.uint16) == SENTINEL).any()
    with pytest.raises(Exception):
        ctx.skybox_bc6h(g, tile, dev[:5], size, mips, sten, W, out, W)
    with pytest.raises(Exception):
        ctx.skybox_bc6h(g, tile, [d[:n] for d in dev], size, mips + 1, sten, W, out, W)


def test_frames_with_a_resident_sky(ctx, fixture, ibl):
    """DeferredFrame.set_sky_file(data, resident=True): HDR and LDR equal the resident=False frame's bit for bit, also with
    recompute_sh=True, where the SH pack is equal as well; frame.sky holds the uploaded file and no fp32 cube; sky_cube() hands
    prefilter_env a decoded cube equal to the non-resident frame's; a two-view MultiViewFrame with the resident sky equals its
    decoded twin"""
    from direct12pbrrenderer_amd.pipeline import DeferredFrame, MultiViewFrame, ResidentSky, TileSpec
    import camera_cases
    data = fixture["smooth_file"].tobytes()
    size, mips, _, _ = host.parse_cubemap_file(data)
    _, env, lut, sh = ibl
    W, H = 128, 72
    cam, g, lights, gb, tile = common.shade_scene(W, H, 16, sh, coverage_mask=True)

    def dev_half(a):
        return ctx.upload(np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)).view(torch.float16)

    def frame(resident, recompute_sh):
        fr = DeferredFrame(ctx, TileSpec(0, 0, W, H, W, H, 0), g, lights, dev_half(lut), lut.shape[0], dev_half(env), common.ENV_SIZE, common.ENV_MIPS)
        fr.upload_gbuffer(gb)
        fr.set_prev_luminance(0.18)
        pack = fr.set_sky_file(data, recompute_sh=recompute_sh, resident=resident)
        fr.render()
        ctx.sync()
        return fr, np.asarray(pack, np.float32), to_half(fr.hdr).view(np.uint16), fr.ldr_numpy()

    assert (gb["stencil"] == 0).sum() > 500
    for recompute_sh in (False, True):
        fa, sh_a, hdr_a, ldr_a = frame(False, recompute_sh)
        fb, sh_b, hdr_b, ldr_b = frame(True, recompute_sh)
        assert np.array_equal(hdr_a, hdr_b) and np.array_equal(ldr_a, ldr_b), recompute_sh
        assert np.array_equal(sh_a.view(np.uint32), sh_b.view(np.uint32)) and bytes(fa.g.SkyBoxSH) == bytes(fb.g.SkyBoxSH)
        assert isinstance(fb.sky, ResidentSky) and not isinstance(fa.sky, ResidentSky)
        held = [v for v in vars(fb.sky).values() if torch.is_tensor(v)]
        assert [t.dtype for t in held] == [torch.uint8] and held[0].numel() == len(data)           # the file, and no fp32 cube
        assert hdr_b[gb["stencil"] == 0][:, :3].max() > 0
    cube_b, s_b, m_b = fb.sky_cube()
    assert (s_b, m_b) == (size, mips) and torch.equal(cube_b.view(torch.int32), fa.sky[0].view(torch.int32))
    assert fa.sky_cube()[0] is fa.sky[0]
    env_a, env_b = ctx.prefilter_env(fa.sky[0], size, mips, 32, 4), ctx.prefilter_env(cube_b, size, mips, 32, 4)
    ctx.sync()
    assert np.array_equal(to_half(env_a).view(np.uint16), to_half(env_b).view(np.uint16))

    # two views
    names = ("default", "pitch_roll")
    globals_ = [camera_cases.make_global(n, W, H, sh)[1] for n in names]
    gbs = [synth.gbuffer_tile(0, 0, W, H, W, H, coverage_mask=True) for _ in names]
    out = {}
    for what, sky in (("decoded", fa.sky), ("resident", fb.sky)):
        mv = MultiViewFrame(ctx, W, H, globals_, [lights, lights[:5]], dev_half(lut), lut.shape[0], dev_half(env), common.ENV_SIZE,
                            common.ENV_MIPS, sky=sky)
        mv.upload_gbuffers(gbs)
        mv.set_prev_luminance(0.18)
        mv.render()
        ctx.sync()
        out[what] = [(to_half(mv.hdr(v)).view(np.uint16), mv.ldr[v].cpu().numpy()) for v in range(2)]
    for v in range(2):
        assert np.array_equal(out["decoded"][v][0], out["resident"][v][0]) and np.array_equal(out["decoded"][v][1], out["resident"][v][1]), v
    assert not np.array_equal(out["resident"][0][0], out["resident"][1][0])


def test_host_graph_with_a_resident_sky(ctx, fixture):
    """set_skybox_file(data, resident=True) through libpbr_host.so, dispatch by dispatch and fused, the prefilter pass included: the
    render target, the LDR image and the SH pack equal the non-resident renderer's bit for bit (recompute_sh too);
    pbrh_sky_resident_bytes is the file's byte count (padded to the allocation granularity at most) where the non-resident renderer
    holds at least 16 * pbr_cube_texels"""
    data = fixture["smooth_file"].tobytes()
    size, mips, _, _ = host.parse_cubemap_file(data)
    W, H = 160, 96
    gb = synth.gbuffer_tile(0, 0, W, H, W, H, coverage_mask=True)
    assert (gb["stencil"] == 0).sum() > 500

    def frames(resident, fused, recompute_sh):
        q = host.HostRenderer(0, W, H, 16, 32)
        try:
            q.set_fused(fused)
            q.set_skybox_file(data, recompute_sh=recompute_sh, resident=resident)
            q.set_gbuffer(gb)
            q.set_initial_luminance(0.18)
            q.render(1.0 / 60.0)
            q.render(1.0 / 60.0)
            g = Global()
            assert q.lib.pbrh_get_global(q.h, C.addressof(g)) == 0
            return (bytes(g.SkyBoxSH), q.read("DeferredShadingRT", (H, W, 4), np.float16).view(np.uint16),
                    q.read("ToneMappedTexture", (H, W), np.uint32), q.sky_resident_bytes())
        finally:
            q.close()

    for fused, recompute_sh in ((False, False), (True, False), (True, True)):
        sh_a, hdr_a, ldr_a, bytes_a = frames(False, fused, recompute_sh)
        sh_b, hdr_b, ldr_b, bytes_b = frames(True, fused, recompute_sh)
        assert sh_a == sh_b, (fused, recompute_sh)
        assert np.array_equal(hdr_a, hdr_b) and np.array_equal(ldr_a, ldr_b), (fused, recompute_sh)
        assert hdr_b[gb["stencil"] == 0][:, :3].max() > 0 and hdr_b[gb["stencil"] != 0][:, :3].max() > 0      # sky and shade (the env chain) both drew
        assert len(data) <= bytes_b <= len(data) + 4096 and bytes_a >= 16 * cube_texels(size, mips), (bytes_a, bytes_b)
    q = host.HostRenderer(0, W, H, 16, 32)
    try:
        assert q.sky_resident_bytes() == 0                                           # no sky yet
        with pytest.raises(host.HostError, match="truncated"):
            q.set_skybox_file(data[:-5], resident=True)
    finally:
        q.close()
