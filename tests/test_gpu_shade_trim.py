"""k_deferred_shade after the trim of its walk and of its per-row code: lists padded to a multiple of four entries and walked two trips
per step; column terms evaluated once per thread, row terms once per block row.  Every case compares pbr_deferred_shade_f32 with the
oracle under the shade's parity criterion, per pixel and channel
    |gpu - truth| <= 1e-4 * scale + 4 * |fp32 restatement - truth|
(truth: the double-precision evaluation, scale: its largest value over the tile); where two GPU launches must agree they agree bit
for bit.  The frame is 1920 x 1080, so the cluster grid is the real 24 x 16 x 8 one; the shaded tiles are small."""
import numpy as np
import pytest
import torch

import common
from direct12pbrrenderer_amd import scene, synth
from direct12pbrrenderer_amd.pipeline import MultiViewFrame
from direct12pbrrenderer_amd.structs import CLUSTER_DTYPE, Tile

pytestmark = pytest.mark.gpu

W, H = 1920, 1080
CX, CY, CZ = 24, 16, 8
ES, EM = common.ENV_SIZE, common.ENV_MIPS
BAND = (0, 256, 1024, 32)        # x0, y0, w, h: the launch the tile below is cut out of
TILE = (509, 263, 301, 19)       # two column blocks (256 + 45), long and one-row blocks
PAD_TILE = (800, 544, 64, 8)     # one wave wide, inside cluster tile (10, 7): columns 800 .. 879, rows 540 .. 607
PAD_LENGTHS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 30, 31, 32)


def dev_half(ctx, arr):
    return ctx.upload(np.ascontiguousarray(arr, dtype=np.float16).view(np.uint16)).view(torch.float16)


def cut(gb, outer, inner):
    """the planes of tile `inner` out of those of tile `outer` (both x0, y0, w, h in frame pixels)"""
    x, y = inner[0] - outer[0], inner[1] - outer[1]
    return {k: np.ascontiguousarray(v[y:y + inner[3], x:x + inner[2]]) for k, v in gb.items()}


@pytest.fixture(scope="module")
def world(ctx, orc, ibl):
    """the 1080p frame's camera, the oracle's cluster lists per light count, the band's G-buffer and the device tables: made once"""
    sky, env, lut, sh = ibl
    cam = scene.Camera.reference_default(W, H)
    g = scene.make_global(cam, W, H, sh_pack=sh)
    w = dict(g=g, cam=cam, sh=sh, env=env, lut=lut, dlut=dev_half(ctx, lut), denv_plain=dev_half(ctx, env))
    w["denv"] = ctx.env_pad(w["denv_plain"], ES, EM)
    w["band_gb"] = synth.gbuffer_tile(*BAND, W, H, rough_min=48, coverage_mask=True)
    w["lights"] = {}
    for n in (0, 1, 256, 300):
        lights = common.shade_scene(8, 8, n, sh, full=(W, H))[2]
        cl = orc.cluster_build(g)
        orc.cluster_cull(g, lights, cl)
        w["lights"][n] = (lights, cl)
    return w


def shade_f32(ctx, w, g, rect, gb, cl, lights, full=(W, H)):
    tile = Tile(rect[0], rect[1], rect[2], rect[3], full[0], full[1])
    gbd = {k: ctx.upload(v) for k, v in gb.items()}
    out = ctx.zeros((rect[3], rect[2], 4), torch.float32)
    ctx.deferred_shade_f32(g, tile, gbd, rect[2], w["dlut"], w["lut"].shape[0], w["denv"], ES, EM,
                           ctx.upload(cl), ctx.upload(lights) if len(lights) else None, len(lights), out, rect[2])
    return out.cpu().numpy()


def shade_f16(ctx, w, g, rect, gb, cl_dev, lights_dev, n_lights, rects=None, prefill=0.0):
    tile = Tile(rect[0], rect[1], rect[2], rect[3], W, H)
    gbd = {k: ctx.upload(v) for k, v in gb.items()}
    out = torch.full((rect[3], rect[2], 4), prefill, dtype=torch.float16, device=ctx.torch_device)
    args = (g, tile, gbd, rect[2], w["dlut"], w["lut"].shape[0], w["denv"], ES, EM, cl_dev, lights_dev, n_lights, out, rect[2])
    if rects is None:
        ctx.deferred_shade(*args)
    else:
        ctx.deferred_shade_rects(*args, rects)
    return out.view(torch.int16).cpu().numpy()


def check_vs_oracle(orc, w, g, rect, gb, cl, lights, got, what, full=(W, H)):
    """|gpu - truth| <= 1e-4 scale + 4 |restatement - truth| on every pixel that has one truth; the others (a cluster cell or an
    octahedral fold decided by rounding) against the fp32 restatement under the same bound, all but a handful"""
    tile = Tile(rect[0], rect[1], rect[2], rect[3], full[0], full[1])
    _, want = orc.deferred_shade(g, tile, gb, w["lut"], w["env"], ES, EM, cl, lights, want_f32=True)
    lo, hi, flags = orc.deferred_shade_f64(g, tile, gb, w["lut"], w["env"], ES, EM, cl, lights)
    on = gb["stencil"] > 0
    ok = (flags == 0)[on]
    assert on.sum() >= 0.5 * on.size and ok.mean() >= 0.9, f"{what}: too few pixels to compare"
    assert np.isfinite(got[on]).all(), what
    scale = float(np.abs(hi[on][ok]).max())
    d_orc, d_gpu = orc.truth_distance(want, lo, hi)[on], orc.truth_distance(got, lo, hi)[on]
    bound = 1e-4 * scale + 4.0 * d_orc
    worst = (d_gpu / bound)[ok]
    print(f"[shade trim] {what}: {int(ok.sum())} pixels, worst {worst.max():.3f} x the bound (gpu {d_gpu[ok].max() / scale:.3g}, restatement {d_orc[ok].max() / scale:.3g} of scale {scale:.4g})", flush=True)
    assert (worst <= 1.0).all(), f"{what}: a pixel is {worst.max():.2f} x its bound from the exact value"
    off = (np.abs(got[on][:, :3].astype(np.float64) - want[on][:, :3]) > bound).any(axis=1) & ~ok
    assert off.sum() <= max(2, int(1e-4 * on.sum())), f"{what}: {int(off.sum())} edge pixels differ from the fp32 restatement"
    assert np.all(got[on][:, 3] == 1.0) and np.all(got[~on] == 0.0), what


@pytest.fixture(scope="module")
def pad_scene(world):
    """the 64 x 8 tile's G-buffer and the slices of cluster tile (10, 7) its pixels fall into (ClusterIndex in double: only used to
    say which slice holds the most pixels)"""
    gb = synth.gbuffer_tile(*PAD_TILE, W, H, rough_min=48, coverage_mask=True)
    g = world["g"]
    near, far = float(g.Near), float(g.Far)
    z = near * far / (far - gb["depth"].astype(np.float64) * (far - near))
    sz = np.clip((CZ * np.log(np.clip(z, near, far) / near) / np.log(far / near)).astype(np.int64), 0, CZ - 1)
    xs, ys = np.arange(PAD_TILE[0], PAD_TILE[0] + PAD_TILE[2]), np.arange(PAD_TILE[1], PAD_TILE[1] + PAD_TILE[3])
    assert set(np.floor((xs + 0.5) / W * CX).astype(int)) == {10} and set(np.floor((1 - (ys + 0.5) / H) * CY).astype(int)) == {7}
    return gb, sz, gb["stencil"] > 0


@pytest.mark.parametrize("length", PAD_LENGTHS)
def test_padded_lists_of_every_length(ctx, orc, world, pad_scene, length):
    """The slice that holds most of the tile's pixels gets a list of `length` entries, its neighbours the other lengths in turn: the
    lanes of a wave leave the walk after different trips, and every length is padded to its multiple of four with the null light."""
    gb, sz, on = pad_scene
    lights, cl0 = world["lights"][256]
    cl = np.array(cl0, copy=True)
    clv = cl.view(CLUSTER_DTYPE).reshape(-1)
    used = np.bincount(sz[on], minlength=CZ)
    main = int(used.argmax())
    assert (used > 0).sum() >= 2 and (np.array([len(set(r[m])) for r, m in zip(sz, on)]) >= 2).any(), "one wave must hold two slices"
    i = PAD_LENGTHS.index(length)
    rng = np.random.default_rng(1234 + length)
    for z in range(CZ):
        c = z + 10 * CZ + 7 * CX * CZ
        clv["NumLights"][c] = PAD_LENGTHS[(i + z - main) % len(PAD_LENGTHS)]
        clv["LightIndex"][c] = rng.permutation(len(lights))[:32]
    assert clv["NumLights"][main + 10 * CZ + 7 * CX * CZ] == length
    got = shade_f32(ctx, world, world["g"], PAD_TILE, gb, cl, lights)
    check_vs_oracle(orc, world, world["g"], PAD_TILE, gb, cl, lights, got, f"list of {length}")


@pytest.fixture(scope="module")
def band(ctx, orc, world):
    """the 1024 x 32 launch, compared with the oracle once"""
    lights, cl = world["lights"][256]
    got = shade_f32(ctx, world, world["g"], BAND, world["band_gb"], cl, lights)
    check_vs_oracle(orc, world, world["g"], BAND, world["band_gb"], cl, lights, got, "band 1024x32")
    return got


def test_column_origin_tile_equals_the_band(ctx, orc, world, band):
    lights, cl = world["lights"][256]
    gb = cut(world["band_gb"], BAND, TILE)
    got = shade_f32(ctx, world, world["g"], TILE, gb, cl, lights)
    check_vs_oracle(orc, world, world["g"], TILE, gb, cl, lights, got, "tile 301x19 at (509, 263)")
    x, y = TILE[0] - BAND[0], TILE[1] - BAND[1]
    assert np.array_equal(got.view(np.uint32), band[y:y + TILE[3], x:x + TILE[2]].view(np.uint32)), "the tile differs from the same pixels of the band"


def test_column_origin_rectangles(ctx, world):
    """the tile's pixels as three rectangles of different x in ONE launch over the band: the bits of the whole-band launch, nothing else touched"""
    lights, cl = world["lights"][256]
    dl, dc = ctx.upload(lights), ctx.upload(cl)
    whole = shade_f16(ctx, world, world["g"], BAND, world["band_gb"], dc, dl, len(lights))
    x, y = TILE[0] - BAND[0], TILE[1] - BAND[1]
    rects = [(x, y, 77, TILE[3]), (x + 77, y, 131, TILE[3]), (x + 208, y, 93, TILE[3])]
    assert sum(r[2] * r[3] for r in rects) == TILE[2] * TILE[3]
    got = shade_f16(ctx, world, world["g"], BAND, world["band_gb"], dc, dl, len(lights), rects=rects, prefill=7.0)
    inside = np.zeros(got.shape[:2], dtype=bool)
    inside[y:y + TILE[3], x:x + TILE[2]] = True
    on = world["band_gb"]["stencil"] > 0
    assert np.array_equal(got[inside & on], whole[inside & on]), "rectangles differ from the whole band"
    assert np.all(got[~(inside & on)] == np.float16(7.0).view(np.int16)), "a pixel outside the rectangles was written"


def test_column_origin_two_views(ctx, world):
    """two whole 1080p frames with different cameras in one launch: each view's tile pixels equal the single launch over the band"""
    ins = []
    for v in range(2):
        if v == 0:
            g, lights = world["g"], world["lights"][256][0]
            gb = synth.gbuffer_tile(0, 0, W, H, W, H, rough_min=48, coverage_mask=True)
        else:
            cam = scene.Camera(np.float32(0.373) * np.float32(np.pi), W, H, 0.25, 400.0)
            cam.move((0.3, 3.0, 9.5))
            cam.rotate(0.0, float(np.pi) + 0.15, 0.0)
            g = scene.make_global(cam, W, H, sh_pack=world["sh"])
            lights = synth.lights_in_view_box(256, cam, seed=0x5EED0101)
            gb = synth.gbuffer_tile(0, 0, W, H, W, H, near=0.25, far=400.0, rough_min=48, coverage_mask=True, cell=2)
        ins.append((g, lights, gb))
    mv = MultiViewFrame(ctx, W, H, [i[0] for i in ins], [i[1] for i in ins], world["dlut"], world["lut"].shape[0], world["denv_plain"], ES, EM)
    mv.upload_gbuffers([i[2] for i in ins])
    mv.clustered()
    mv.shade()
    ctx.sync()
    x, y = TILE[0], TILE[1]
    cuts = []
    for v, (g, lights, gb) in enumerate(ins):
        view = mv.hdr(v).view(torch.int16).cpu().numpy()[y:y + TILE[3], x:x + TILE[2]]
        single = shade_f16(ctx, world, g, BAND, cut(gb, (0, 0, W, H), BAND), mv.clusters[v], ctx.upload(lights), len(lights))
        on = gb["stencil"][y:y + TILE[3], x:x + TILE[2]] > 0
        assert on.sum() > 0.5 * on.size
        assert np.array_equal(view[on], single[y - BAND[1]:y - BAND[1] + TILE[3], x:x + TILE[2]][on]), f"view {v} differs from its single launch"
        cuts.append(view)
    assert not np.array_equal(cuts[0], cuts[1]), "the views must differ from each other"


@pytest.mark.parametrize("n_lights", [0, 1, 300])
def test_other_light_counts(ctx, orc, world, n_lights):
    """no lights (every list one null group), one light, and 300: the 1025-stride light table"""
    lights, cl = world["lights"][n_lights]
    assert len(lights) == n_lights
    gb = cut(world["band_gb"], BAND, TILE)
    got = shade_f32(ctx, world, world["g"], TILE, gb, cl, lights)
    check_vs_oracle(orc, world, world["g"], TILE, gb, cl, lights, got, f"tile 301x19, {n_lights} lights")


def test_small_frame_takes_the_global_lists(ctx, orc, world):
    """96 x 54 shaded whole: a block spans more cluster tiles than it may stage, so the walk reads the global lists"""
    cam, g, lights, gb, tile = common.shade_scene(96, 54, 256, world["sh"], rough_min=48)
    cl = orc.cluster_build(g)
    orc.cluster_cull(g, lights, cl)
    got = shade_f32(ctx, world, g, (0, 0, 96, 54), gb, cl, lights, full=(96, 54))
    check_vs_oracle(orc, world, g, (0, 0, 96, 54), gb, cl, lights, got, "frame 96x54", full=(96, 54))

