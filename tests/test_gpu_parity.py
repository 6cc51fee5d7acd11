"""GPU parity: every HIP kernel, called through the C ABI (libpbr_hip.so), against the CPU oracle
on the same seeded inputs and against the committed golden fixtures.

Tolerances: LUT <= 1 fp16 ULP; prefiltered env <= 1 fp16 ULP or 1e-3 rel; shaded HDR
<= 1e-4 relative L-inf (relative to the frame's max radiance) and <= a few fp16 ULP per texel; bloom
stages bit-exact (the bloom TU is built -ffp-contract=off in the oracle's operation order);
histogram exact up to boundary flips <= 1e-5 N; average luminance exact given an equal histogram;
RGBA8 <= 1 LSB; SH <= 1e-5 relative.
"""
import numpy as np
import pytest
import torch

import common
from direct12pbrrenderer_amd import scene, synth
from direct12pbrrenderer_amd.structs import CLUSTER_DTYPE, Tile, bloom_level_offset, cube_mip_offset
from shade_checks import _check_shade, _check_shade_f32, assert_half_close

pytestmark = pytest.mark.gpu


def dev_half(ctx, arr):
    return ctx.upload(np.ascontiguousarray(arr, dtype=np.float16).view(np.uint16)).view(torch.float16)


def to_np_half(t):
    return t.cpu().view(torch.int16).numpy().view(np.float16)


# ------------------------------------------------------------------------------------------ a3
@pytest.mark.parametrize("res", [32, 256])
def test_brdf_lut_vs_oracle(ctx, orc, golden, res):
    got = to_np_half(ctx.brdf_lut(res))
    if res == 32:
        want = orc.brdf_lut(32)
        assert np.array_equal(want, golden["lut32"])
        assert_half_close(got, want, 1, "LUT 32")
    else:
        for r in (0, 100, 255):
            assert_half_close(got[r], golden[f"lut256_row{r}"], 1, f"LUT 256 row {r}")
        rows = orc.brdf_lut_rows(256, 37, 2)
        assert_half_close(got[37:39], rows, 1, "LUT 256 rows 37-38")


def test_brdf_lut_512_reference_default(ctx, golden):
    # the reference's real LUT size (DeferredPipeline.h:80,85)
    got = to_np_half(ctx.brdf_lut(512))
    for r in (0, 255, 511):
        assert_half_close(got[r], golden[f"lut512_row{r}"], 1, f"LUT 512 row {r}")
    # analytic column: roughness 0 => A = 1-(1-NdotV)^5, B = (1-NdotV)^5
    ndv = (np.arange(512) + 1) / 512
    B = (1 - ndv) ** 5
    assert np.abs(got[:, 0, 0].astype(np.float64) - (1 - B)).max() <= 5e-4
    assert np.abs(got[:, 0, 1].astype(np.float64) - B).max() <= 5e-4


@pytest.mark.parametrize("res", [256, 512])
def test_brdf_lut_whole_plane_vs_oracle(ctx, orc, golden2, res):
    """cfg1 (256^2) and the reference's real size (512^2): EVERY texel within 1 fp16 ULP of the oracle plane, whose
    CRC and 64 sampled texels are pinned by tests/golden/golden_v2.npz."""
    import zlib
    want = orc.brdf_lut(res)
    assert np.uint32(zlib.crc32(np.ascontiguousarray(want).tobytes())) == golden2[f"lut{res}_crc"]
    got = to_np_half(ctx.brdf_lut(res))
    d = common.half_ulp_diff(got, want)
    assert d.max() <= 1, f"LUT {res}: max {d.max()} ULP, {(d > 1).sum()} texels over"
    idx = golden2[f"lut{res}_idx"]
    assert common.half_ulp_diff(got.reshape(-1, 2)[idx], golden2[f"lut{res}_texels"]).max() <= 1
    print(f"LUT {res}^2: {(d == 0).mean() * 100:.2f} % of the plane bit-identical to the oracle, max 1 ULP")


@pytest.mark.parametrize("res", [256, 512])
def test_brdf_lut_against_the_double_precision_truth(ctx, orc, res):
    """The LUT kernel's sample step is algebraically rearranged (no normalize(L), the floor of NdotH NdotV as a min of
    reciprocals, fused multiply-adds, clamp modifiers): besides staying within 1 fp16 ULP of the fp32 restatement of the shader's
    order of operations (above), it is checked against the estimator evaluated in DOUBLE (oracle/pbr_oracle_f64.cpp
    orc_brdf_lut_f64) — per texel no further from the correctly rounded truth than the fp32 restatement is, plus one ULP.
    (The fp32 shader arithmetic itself is up to 7 ULP off the truth in a handful of texels at NdotV <= 2 / res and roughness
    < 0.06: sin(theta) = sqrt(1 - cos^2) of the GGX sample cancels there; the kernel builds its table with that same arithmetic.)"""
    truth = orc.brdf_lut_f64(res).astype(np.float16)
    want = orc.brdf_lut(res)
    got = to_np_half(ctx.brdf_lut(res))
    dg, do = common.half_ulp_diff(got, truth), common.half_ulp_diff(want, truth)
    assert (dg <= do + 1).all(), f"LUT {res}: {(dg > do + 1).sum()} texels further from the f64 truth than the fp32 restatement + 1 ULP (worst {int((dg - do).max())})"
    print(f"LUT {res}^2 vs round(f64): kernel {(dg == 0).mean() * 100:.3f} % exact, max {int(dg.max())} ULP, {(dg > 1).sum()} texels > 1 ULP | "
          f"fp32 restatement {(do == 0).mean() * 100:.3f} % exact, max {int(do.max())} ULP, {(do > 1).sum()} texels > 1 ULP")


def test_prefilter_env_512_and_sh9_vs_fixture(ctx, orc, golden2):
    """cfg3 at its stated size: 512^2 cube, 5 mips, 1024 spp + SH9.  The CPU cannot afford the whole chain (2.1e9
    sample steps), so 4096 seeded texels across the five mips are compared: fixture (generated in the build container)
    and the live oracle on the box."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_v2 as mk
    sky = mk.bench_sky()
    dsky = ctx.upload(sky)
    got = to_np_half(ctx.prefilter_env(dsky, mk.ENV_SIZE, mk.SKY_MIPS, mk.ENV_SIZE, mk.ENV_MIPS))
    worst = 0
    for m in range(mk.ENV_MIPS):
        idx = golden2[f"env512_m{m}_idx"]
        want = golden2[f"env512_m{m}_texels"]
        live = orc.prefilter_env_texels(sky, mk.ENV_SIZE, mk.SKY_MIPS, mk.ENV_SIZE, mk.ENV_MIPS, m, idx[::4])
        assert np.array_equal(live.view(np.uint16), want[::4].view(np.uint16)), f"mip {m}: oracle on this host differs from the fixture"
        sub = got[cube_mip_offset(mk.ENV_SIZE, m) + idx.astype(np.int64)]
        d = common.half_ulp_diff(sub, want)
        ok = (d <= 1) | (np.abs(sub.astype(np.float32) - want.astype(np.float32)) <= 1e-3 * np.abs(want.astype(np.float32)))
        assert ok.all(), f"prefilter 512^2 mip {m}: {(~ok).sum()} of {len(idx)} texels outside 1 ULP / 1e-3"
        worst = max(worst, int(d.max()))
        assert np.all(sub[:, 3] == 1.0)
    print(f"prefilter 512^2 x 5: 4096 sampled texels, worst {worst} fp16 ULP")
    sh = ctx.sh9_project(dsky, mk.ENV_SIZE, mk.SKY_MIPS).cpu().numpy()
    assert np.abs(sh - golden2["sh512"]).max() <= 1e-5 * np.abs(golden2["sh512"]).max()


def test_brdf_lut_bad_args(ctx):
    from direct12pbrrenderer_amd.api import PbrError
    with pytest.raises(PbrError):
        ctx.brdf_lut(1, out=ctx.empty((4,), torch.float16))


# ------------------------------------------------------------------------------------------ cube mips / a4 / a5
def test_cube_gen_mips_bit_exact(ctx, orc):
    sky = synth.env_cube(32, 6)
    want = orc.cube_gen_mips(sky.copy(), 32, 6)
    d = ctx.upload(sky)
    ctx.cube_gen_mips(d, 32, 6)
    assert np.array_equal(d.cpu().numpy(), want)


def test_prefilter_env_vs_oracle_and_golden(ctx, orc, golden, ibl):
    sky, env, _, _ = ibl
    got = to_np_half(ctx.prefilter_env(ctx.upload(sky), common.SKY_SIZE, common.SKY_MIPS, common.ENV_SIZE, common.ENV_MIPS))
    assert np.array_equal(env, golden["env16"])
    g32, w32 = got.astype(np.float32), env.astype(np.float32)
    ok = (common.half_ulp_diff(got, env) <= 1) | (np.abs(g32 - w32) <= 1e-3 * np.abs(w32))
    assert ok.all(), f"prefilter: {(~ok).sum()} texels outside 1 ULP / 1e-3"
    assert np.all(got[:, 3] == 1.0)


def test_prefilter_env_per_dispatch_kernel_vs_oracle(ctx, orc, ibl):
    """pbr_prefilter_env_mip — one reference dispatch, the shader's strictly sequential sum (what the C++ pass graph
    issues five times) — against the oracle, all five mips of the 16^2 chain."""
    sky, env, _, _ = ibl
    got = to_np_half(ctx.prefilter_env_dispatches(ctx.upload(sky), common.SKY_SIZE, common.SKY_MIPS, common.ENV_SIZE, common.ENV_MIPS))
    ok = (common.half_ulp_diff(got, env) <= 1) | (np.abs(got.astype(np.float32) - env.astype(np.float32)) <= 1e-3 * np.abs(env.astype(np.float32)))
    assert ok.all(), f"prefilter (per dispatch): {(~ok).sum()} texels outside 1 ULP / 1e-3"
    assert (common.half_ulp_diff(got, env) == 0).mean() > 0.99      # same summation order: nearly every texel bit-identical


def test_prefilter_env_larger_cube_one_mip(ctx, orc):
    # 64^2 source, 32^2 output mip 2 (roughness 0.5): exercises PDF-based LOD selection across mips
    sky = synth.env_cube(64, 7)
    orc.cube_gen_mips(sky, 64, 7)
    got = to_np_half(ctx.prefilter_env(ctx.upload(sky), 64, 7, 128, 5))
    m = 2
    want = orc.prefilter_env_mip(sky, 64, 7, 128, 5, m)
    off = cube_mip_offset(128, m)
    sub = got[off: off + want.shape[0]]
    ok = (common.half_ulp_diff(sub, want) <= 1) | (np.abs(sub.astype(np.float32) - want.astype(np.float32)) <= 1e-3 * np.abs(want.astype(np.float32)))
    assert ok.all()


def test_sh9_vs_oracle(ctx, orc, golden, ibl):
    sky = ibl[0]
    got = ctx.sh9_project(ctx.upload(sky), common.SKY_SIZE, common.SKY_MIPS).cpu().numpy()
    want = orc.sh9_project(sky, common.SKY_SIZE)
    assert np.array_equal(want, golden["sh16"])
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-5 * scale
    # 128^2 cube (98 304 texels -> multi-block reduction)
    sky2 = synth.env_cube(128, 1)
    got2 = ctx.sh9_project(ctx.upload(sky2), 128, 1).cpu().numpy()
    want2 = orc.sh9_project(sky2, 128)
    assert np.abs(got2 - want2).max() <= 1e-5 * np.abs(want2).max()


# ------------------------------------------------------------------------------------------ a13
def _clusters_from_dev(t):
    return np.frombuffer(t.cpu().numpy().tobytes(), dtype=CLUSTER_DTYPE).copy()


def test_cluster_build_and_cull(ctx, orc, golden, ibl):
    cam, g, lights, gb, tile = common.shade_scene(64, 64, 256, ibl[3])
    want = orc.cluster_build(g)
    d = ctx.alloc_clusters()
    ctx.cluster_build(g, d)
    got = _clusters_from_dev(d)
    for k in ("MinBound", "MaxBound"):
        assert np.allclose(got[k], want[k], rtol=2e-6, atol=1e-7), k     # powf/tanf are libm-class on both sides
    assert np.all(got["NumLights"] == 0)
    # cull on the ORACLE's boxes must give the identical light lists (integer output)
    d2 = ctx.upload(want)
    ctx.cluster_cull(g, ctx.upload(lights), len(lights), d2)
    got2 = _clusters_from_dev(d2)
    orc.cluster_cull(g, lights, want)
    assert np.array_equal(got2["NumLights"], want["NumLights"])
    assert np.array_equal(want["NumLights"], golden["clusters_l256_numlights"])
    mask = np.arange(32)[None, :] < want["NumLights"][:, None]
    assert np.array_equal(got2["LightIndex"][mask], want["LightIndex"][mask])
    assert want["NumLights"].max() == 32 and (want["NumLights"] == 0).any()   # cap and empties both exercised
    # cull on the GPU-built boxes: ULP-level box differences may flip only borderline lights
    ctx.cluster_cull(g, ctx.upload(lights), len(lights), d)
    got3 = _clusters_from_dev(d)
    assert (got3["NumLights"] != want["NumLights"]).mean() <= 0.002


def test_cluster_cull_edge_cases(ctx, orc, ibl):
    from direct12pbrrenderer_amd.api import PbrError
    cam, g, lights, gb, tile = common.shade_scene(64, 64, 1, ibl[3])
    d = ctx.alloc_clusters()
    ctx.cluster_build(g, d)
    ctx.cluster_cull(g, None, 0, d)                       # zero lights is legal
    assert np.all(_clusters_from_dev(d)["NumLights"] == 0)
    with pytest.raises(PbrError):
        ctx.cluster_cull(g, ctx.upload(lights), 1025, d)  # > MaxSceneLights (DeferredPipeline.cpp:222)
    # 1024 lights, the reference's maximum
    many = synth.lights_in_view_box(1024, cam)
    want = orc.cluster_build(g)
    d2 = ctx.upload(want)
    ctx.cluster_cull(g, ctx.upload(many), 1024, d2)
    orc.cluster_cull(g, many, want)
    got = _clusters_from_dev(d2)
    assert np.array_equal(got["NumLights"], want["NumLights"])
    mask = np.arange(32)[None, :] < want["NumLights"][:, None]
    assert np.array_equal(got["LightIndex"][mask], want["LightIndex"][mask])


# ------------------------------------------------------------------------------------------ a8-a12
def _shade_on_gpu(ctx, g, tile, gb, lut, env, env_size, env_mips, clusters_np, lights, prefill=None):
    h, w = gb["A"].shape
    gbd = {k: ctx.upload(v) for k, v in gb.items()}
    hdr = ctx.zeros((h, w, 4), torch.float16) if prefill is None else dev_half(ctx, prefill)
    env_padded = ctx.env_pad(dev_half(ctx, env), env_size, env_mips)
    ctx.deferred_shade(g, tile, gbd, w, dev_half(ctx, lut), lut.shape[0], env_padded, env_size, env_mips,
                       ctx.upload(clusters_np), ctx.upload(lights) if len(lights) else None, len(lights), hdr, w)
    return to_np_half(hdr)


def _truth(orc, g, tile, gb, lut, env, env_size, env_mips, cl, lights):
    """The shade in DOUBLE precision (oracle/pbr_oracle_f64.cpp): per-channel interval [lo, hi] of the exact value of the
    reference's formulas on these inputs (lo == hi away from sampler-step / cube-face edges) + flags (0 = comparable)."""
    return orc.deferred_shade_f64(g, tile, gb, lut, env, env_size, env_mips, cl, lights)


@pytest.mark.parametrize("n_lights", [0, 1, 256])
def test_deferred_shade_64_vs_oracle_and_golden(ctx, orc, golden, ibl, n_lights):
    sky, env, lut, sh = ibl
    cam, g, lights, gb, tile = common.shade_scene(64, 64, n_lights, sh)
    cl = orc.cluster_build(g)
    orc.cluster_cull(g, lights, cl)
    want, want_f32 = orc.deferred_shade(g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights, want_f32=True)
    assert np.array_equal(want, golden[f"shade64_l{n_lights}"])
    truth = _truth(orc, g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights)
    sentinel = np.full((64, 64, 4), 7.0, dtype=np.float16)
    got = _shade_on_gpu(ctx, g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights, prefill=sentinel)
    _check_shade(orc, got, want, want_f32, truth, gb["stencil"], f"shade {n_lights} lights", rough=gb["C"] & 255)
    assert np.all(got[gb["stencil"] == 0] == 7.0)      # stencil == 0 pixels are left untouched


def test_deferred_shade_ragged_tile_of_a_larger_frame(ctx, orc, ibl):
    # 200 x 37 tile at (328, 91) of a 640 x 360 frame: width not a multiple of 64/256, rows not of 8,
    # global-pixel uv / camera ray / ClusterIndex, pitch > width
    sky, env, lut, sh = ibl
    cam, g, lights, gb, tile = common.shade_scene(200, 37, 256, sh, full=(640, 360), x0=328, y0=91)
    cl = orc.cluster_build(g)
    orc.cluster_cull(g, lights, cl)
    want, want_f32 = orc.deferred_shade(g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights, want_f32=True)
    truth = _truth(orc, g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights)
    got = _shade_on_gpu(ctx, g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights)
    _check_shade(orc, got, want, want_f32, truth, gb["stencil"], "ragged tile", rough=gb["C"] & 255)
    # the same region shaded as part of the whole frame agrees with the tile
    cam2, g2, lights2, gbf, tilef = common.shade_scene(640, 360, 256, sh)
    full = _shade_on_gpu(ctx, g2, tilef, gbf, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights2)
    assert np.array_equal(full[91:91 + 37, 328:328 + 200], got)


# ---- the north_star bound itself: <= 1e-4 relative L-inf on the fp32 colour BEFORE the fp16 store, against the EXACT value
def _shade_f32_on_gpu(ctx, g, tile, gb, dlut, lut_res, env_padded, env_size, env_mips, clusters_np, lights):
    h, w = gb["A"].shape
    gbd = {k: ctx.upload(v) for k, v in gb.items()}
    out = ctx.zeros((h, w, 4), torch.float32)
    ctx.deferred_shade_f32(g, tile, gbd, w, dlut, lut_res, env_padded, env_size, env_mips,
                           ctx.upload(clusters_np), ctx.upload(lights) if len(lights) else None, len(lights), out, w)
    return out.cpu().numpy()


def _dist_line(what, rg, ro):
    q = lambda a: f"max {a.max():.2e}, q99.99 {np.quantile(a, .9999):.1e}, q99 {np.quantile(a, .99):.1e}, > 1e-4: {int((a > 1e-4).sum())}"
    return f"fp32 shade vs f64 truth, {what} ({rg.size} px): GPU {q(rg)} | fp32 restatement {q(ro)}"


@pytest.mark.parametrize("n_lights", [0, 1, 256, 1024])
def test_deferred_shade_f32_within_1e4_relative_linf(ctx, orc, ibl, n_lights):
    """64x64 (0 / 1 / 256 / 1024 lights: the last one runs k_deferred_shade<*, 1025>) and a ragged tile of a larger frame,
    with the throughput frames' roughness range and with the full one (GGX peaks at roughness -> 0)."""
    sky, env, lut, sh = ibl
    dlut, denv = dev_half(ctx, lut), ctx.env_pad(dev_half(ctx, env), common.ENV_SIZE, common.ENV_MIPS)
    for (w, h, full, x0, y0, rm) in ((64, 64, None, 0, 0, 48), (200, 37, (640, 360), 328, 91, 48), (64, 64, None, 0, 0, 0), (200, 37, (640, 360), 328, 91, 0)):
        cam, g, lights, gb, tile = common.shade_scene(w, h, n_lights, sh, full=full, x0=x0, y0=y0, rough_min=rm)
        cl = orc.cluster_build(g)
        orc.cluster_cull(g, lights, cl)
        if n_lights == 1024:
            assert cl["NumLights"].max() == 32 and len(lights) > 256
        _, want_f32 = orc.deferred_shade(g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights, want_f32=True)
        truth = _truth(orc, g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights)
        got = _shade_f32_on_gpu(ctx, g, tile, gb, dlut, lut.shape[0], denv, common.ENV_SIZE, common.ENV_MIPS, cl, lights)
        rg, ro = _check_shade_f32(orc, got, want_f32, truth, gb["stencil"], f"f32 shade {w}x{h}, {n_lights} lights", rough=gb["C"] & 255)
        print(_dist_line(f"{w}x{h}, {n_lights} lights", rg, ro))


@pytest.mark.parametrize("w,h", [(256, 144), (1920, 96)])
def test_deferred_shade_1024_lights_fp16_target(ctx, orc, ibl, w, h):
    """257..1024 scene lights select the kernel instantiation with the 1025-float LDS plane stride.  1920x96: a block spans
    4 x 3 = 12 cluster tiles — within the staging limit, but 36 KiB of light planes + 12 x 24 dword lists pass the 64 KiB a
    block may ask for, so the launch must fall back to the global lists instead of failing."""
    sky, env, lut, sh = ibl
    cam, g, lights, gb, tile = common.shade_scene(w, h, 1024, sh, rough_min=48)
    cl = orc.cluster_build(g)
    orc.cluster_cull(g, lights, cl)
    assert (cl["LightIndex"][cl["NumLights"] > 0].max() > 256)        # lists really index beyond the 257-stride table
    want, want_f32 = orc.deferred_shade(g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights, want_f32=True)
    truth = _truth(orc, g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights)
    got = _shade_on_gpu(ctx, g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights)
    _check_shade(orc, got, want, want_f32, truth, gb["stencil"], f"1024 lights {w}x{h}", hard_ulp=None, rough=gb["C"] & 255)


def test_deferred_shade_rejects_what_its_32bit_offsets_cannot_address(ctx, orc, ibl):
    """The kernel addresses planes, LUT and env chain with 32-bit byte offsets: the host side refuses a LUT above 16384^2 and a
    padded env chain of 4 GiB or more, and says why (nothing is launched)."""
    from direct12pbrrenderer_amd.api import PbrError
    sky, env, lut, sh = ibl
    cam, g, lights, gb, tile = common.shade_scene(64, 64, 1, sh, rough_min=48)
    cl = orc.cluster_build(g)
    orc.cluster_cull(g, lights, cl)
    gbd = {k: ctx.upload(v) for k, v in gb.items()}
    hdr = ctx.zeros((64, 64, 4), torch.float16)
    dlut, denv, dcl, dl = dev_half(ctx, lut), ctx.env_pad(dev_half(ctx, env), common.ENV_SIZE, common.ENV_MIPS), ctx.upload(cl), ctx.upload(lights)
    with pytest.raises(PbrError, match="LUT larger than 16384"):
        ctx.deferred_shade(g, tile, gbd, 64, dlut, 20000, denv, common.ENV_SIZE, common.ENV_MIPS, dcl, dl, len(lights), hdr, 64)
    with pytest.raises(PbrError, match="4 GiB"):
        ctx.deferred_shade(g, tile, gbd, 64, dlut, lut.shape[0], denv, 8192, 1, dcl, dl, len(lights), hdr, 64)
    ctx.deferred_shade(g, tile, gbd, 64, dlut, lut.shape[0], denv, common.ENV_SIZE, common.ENV_MIPS, dcl, dl, len(lights), hdr, 64)   # and accepts the real thing
    ctx.sync()


@pytest.fixture(scope="module")
def bench_ibl(ctx):
    """The IBL bench.py shades with: 512^2 sky -> GPU-built LUT 512^2, prefiltered env 512^2 x 5 mips, SH9 (each
    kernel is oracle-checked on its own: LUT over the whole plane, env on sampled texels of every mip, SH9)."""
    import bench
    lut, env, sh = bench.build_ibl(ctx)
    return lut, env, sh, to_np_half(lut), to_np_half(env)


@pytest.mark.parametrize("w,h,rows", [(1920, 1080, 32), (3840, 2160, 32), (7680, 4320, 16)])
def test_deferred_shade_band_with_the_bench_ibl(ctx, orc, bench_ibl, w, h, rows):
    """A band of the cfg2 / cfg4 frame (256 lights) shaded against the REAL IBL of the bench — LUT 512^2 and the
    512^2 x 5 env chain, not the 16^2 / 32^2 test set — in fp32 (<= 1e-4 rel L-inf) and on the fp16 target.  The oracle
    consumes the very arrays the GPU built, so this checks the shade's sampling of the big chain, not the prefilter."""
    lut_d, env_d, sh, lut, env = bench_ibl
    y0 = (h - rows) // 2 // 8 * 8
    cam, g, lights, gb, tile = common.shade_scene(w, rows, 256, sh, full=(w, h), x0=0, y0=y0, rough_min=48, coverage_mask=False)
    cl = orc.cluster_build(g)
    orc.cluster_cull(g, lights, cl)
    want, want_f32 = orc.deferred_shade(g, tile, gb, lut, env, 512, 5, cl, lights, want_f32=True)
    truth = _truth(orc, g, tile, gb, lut, env, 512, 5, cl, lights)
    envp = ctx.env_pad(env_d, 512, 5)
    got32 = _shade_f32_on_gpu(ctx, g, tile, gb, lut_d, 512, envp, 512, 5, cl, lights)
    rg, ro = _check_shade_f32(orc, got32, want_f32, truth, gb["stencil"], f"{w}x{h} band, bench IBL", rough=gb["C"] & 255)
    print(_dist_line(f"{w}x{rows} band of {w}x{h}, 256 lights, bench IBL", rg, ro))
    gbd = {k: ctx.upload(v) for k, v in gb.items()}
    hdr = ctx.zeros((rows, w, 4), torch.float16)
    ctx.deferred_shade(g, tile, gbd, w, lut_d, 512, envp, 512, 5, ctx.upload(cl), ctx.upload(lights), len(lights), hdr, w)
    _check_shade(orc, to_np_half(hdr), want, want_f32, truth, gb["stencil"], f"{w}x{h} band fp16, bench IBL", hard_ulp=None, rough=gb["C"] & 255)


def test_deferred_shade_full_4k_frame_is_linear_in_the_light_colours(ctx, orc, bench_ibl):
    """Size-independent properties at BASELINE's full size — the whole 3840x2160 / 256-light frame of the bench, every pixel, every cluster
    list, no CPU in the loop (the oracle could not shade 8.3 Mpixel in test time):
      * the light term is LINEAR in the lights' colours, and a factor 1/2 is exact in every product and sum of the walk, so with
        A = no lights (IBL + emission), B = the lights, C = the same lights at half colour:  B - A = 2 (C - A)  to fp32 rounding of the two
        differences — any pixel that walked a wrong or partial list, dropped or doubled a light, or mixed lists between lanes breaks it;
      * black lights add exactly nothing: D = the lights with colour 0 equals A bit for bit (same IBL path, sums of exact zeros);
      * a frame shaded as two half-height tiles equals the frame shaded whole, bit for bit (global pixel coordinates: pbr_tile)."""
    lut_d, env_d, sh, _lut, _env = bench_ibl
    W, H = 3840, 2160
    cam, g, lights, gb, tile = common.shade_scene(W, H, 256, sh, rough_min=48, coverage_mask=False)
    cl = orc.cluster_build(g)
    orc.cluster_cull(g, lights, cl)                      # integer lists: the GPU cull is tested against them elsewhere
    gbd = {k: ctx.upload(v) for k, v in gb.items()}
    envp = ctx.env_pad(env_d, 512, 5)
    cld = ctx.upload(cl)

    def shade(lts, n):
        out = ctx.zeros((H, W, 4), torch.float32)
        ctx.deferred_shade_f32(g, tile, gbd, W, lut_d, 512, envp, 512, 5, cld, ctx.upload(lts), n, out, W)
        ctx.sync()
        return out[..., :3]

    half, black = lights.copy(), lights.copy()
    half["Color"] *= np.float32(0.5)
    black["Color"] = 0.0
    A, B, Cc, D = shade(lights, 0), shade(lights, len(lights)), shade(half, len(lights)), shade(black, len(lights))
    assert bool(torch.isfinite(B).all())
    # with n = 0 the kernel walks null pairs; with black lights it walks the real lists: both must add nothing.  (-0 vs +0 sums aside,
    # compare values, not bits)
    assert bool((A == D).all()), int((A != D).sum())
    scale = float(B.abs().max())
    lhs, rhs = B - A, 2.0 * (Cc - A)
    err = (lhs - rhs).abs()
    # the light term itself scales EXACTLY (power of two); what is left is the rounding of `light + rest` in the kernel's last additions
    # and of the two differences here: a few ulps of the pixel's own magnitude
    tol = 16.0 * torch.finfo(torch.float32).eps * (B.abs() + A.abs()) + 1e-12
    bad = err > tol
    assert not bool(bad.any()), (int(bad.sum()), float(err.max()), scale)
    assert float(lhs.abs().max()) > 0.05 * scale                      # the lights do light the frame
    # two tiles vs the whole frame
    for (y0, hh) in ((0, 1080), (1080, 1080)):
        t = Tile(0, y0, W, hh, W, H)
        sub = {k: ctx.upload(np.ascontiguousarray(v[y0:y0 + hh])) for k, v in gb.items()}
        out = ctx.zeros((hh, W, 4), torch.float32)
        ctx.deferred_shade_f32(g, t, sub, W, lut_d, 512, envp, 512, 5, cld, ctx.upload(lights), len(lights), out, W)
        ctx.sync()
        assert bool(torch.equal(out[..., :3], B[y0:y0 + hh])), (y0, int((out[..., :3] != B[y0:y0 + hh]).sum()))


@pytest.mark.parametrize("size", [16, 32, 64])   # 32: mip 4 is 2 x 2 — its corner texel is an exact three-way face tie for sample 0
def test_prefilter_env_on_a_half_representable_source_takes_the_half_copy_and_stays_within_one_ulp(ctx, orc, size):
    """pbr_prefilter_env samples mips >= 1 from a half-precision copy of the source chain when that copy is exact (what the
    reference's BC6H_UF16 sky assets decode to), from the fp32 chain otherwise.  A source chain rounded to half — every mip,
    as the reference's per-mip block compression leaves it — against the oracle on the same chain: every texel of every mip
    <= 1 fp16 ULP or 1e-3 relative; and the same call on the un-rounded fp32 chain (fp32 path) keeps that bound too."""
    mips = int(np.log2(size)) + 1
    sky = synth.env_cube(size, mips)
    orc.cube_gen_mips(sky, size, mips)
    for name, chain in (("half-representable", sky.astype(np.float16).astype(np.float32)), ("fp32", sky)):
        want = orc.prefilter_env(chain, size, mips, size, 5)
        got = to_np_half(ctx.prefilter_env(ctx.upload(chain), size, mips, size, 5))
        ctx.sync()
        d = common.half_ulp_diff(got[:, :3], want[:, :3])
        rel = np.abs(got[:, :3].astype(np.float32) - want[:, :3].astype(np.float32)) <= 1e-3 * np.abs(want[:, :3].astype(np.float32))
        assert ((d <= 1) | rel).all(), (name, size, int(d.max()))
        assert (d > 0).mean() < 0.25, (name, size, float((d > 0).mean()))


def test_prefilter_env_against_the_double_precision_truth(ctx, orc, golden2):
    """cfg3's 512^2 x 5-mip chain, the 4 096 seeded texels of the fixture: the kernel (v_cube* + v_rcp face coordinates, weight-form
    trilinear sums, the half-precision copy when it is exact) and the fp32 restatement of the shader's arithmetic, each against
    env_map_gen.hlsl evaluated in DOUBLE (oracle/pbr_oracle_f64.cpp orc_prefilter_env_texels_f64: an interval per channel over the
    admissible sides of the x.8 snaps and cube-face ties).  Per texel and channel the kernel's fp16 result lies no further from the
    interval than the restatement's does, plus half an fp16 ULP (one result rounding) and a hundredth for the fp32 sums."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_v2 as mk
    sky = mk.bench_sky()
    for name, chain in (("fp32 source", sky), ("half-representable source", sky.astype(np.float16).astype(np.float32))):
        got = to_np_half(ctx.prefilter_env(ctx.upload(chain), mk.ENV_SIZE, mk.SKY_MIPS, mk.ENV_SIZE, mk.ENV_MIPS))
        worst, inside_g, inside_o, n = 0.0, 0, 0, 0
        for m in range(mk.ENV_MIPS):
            idx = golden2[f"env512_m{m}_idx"][::2]
            lo, hi = orc.prefilter_env_texels_f64(chain, mk.ENV_SIZE, mk.SKY_MIPS, mk.ENV_SIZE, mk.ENV_MIPS, m, idx)
            want = orc.prefilter_env_texels(chain, mk.ENV_SIZE, mk.SKY_MIPS, mk.ENV_SIZE, mk.ENV_MIPS, m, idx)[:, :3].astype(np.float64)
            sub = got[cube_mip_offset(mk.ENV_SIZE, m) + idx.astype(np.int64)][:, :3].astype(np.float64)
            ulp = np.spacing(np.maximum(np.abs(hi), 6.2e-5).astype(np.float16)).astype(np.float64)
            dg = np.maximum(np.maximum(lo - sub, sub - hi), 0.0) / ulp
            do = np.maximum(np.maximum(lo - want, want - hi), 0.0) / ulp
            assert (dg <= do + 0.51).all(), f"{name}, mip {m}: {(dg > do + 0.51).sum()} values further from the f64 interval than the fp32 restatement + 0.51 ULP (worst {float((dg - do).max()):.2f})"
            worst = max(worst, float(dg.max()))
            inside_g += int((dg <= 0.5).sum()); inside_o += int((do <= 0.5).sum()); n += dg.size
        print(f"prefilter 512^2 x 5 vs f64, {name}: kernel within half an fp16 ULP of the interval on {inside_g / n * 100:.2f} % of {n} values "
              f"(fp32 restatement {inside_o / n * 100:.2f} %), worst {worst:.2f} ULP")


def test_prefilter_env_source_levels_above_1670_texels(ctx, orc):
    """k_prefilter_foot forms texel indices in fp32 (exact below 2^24) for source levels up to 1 670 texels and with integer
    multiply-adds above.  A 2 048^2 source filtered into a 32^2 chain puts most samples on source levels 0 (2 048: the integer
    branch) and 1 (1 024: the fp32 branch): 3 x 96 seeded texels against the oracle, on the half-representable chain (half copy
    sampled) and on the fp32 chain (fp32 copy sampled).  The source is the 512^2 synthetic sky repeated 4 x 4 per texel under a
    per-texel modulation (env_cube(2048) itself takes ~20 s of numpy)."""
    S, SM, OUT, MIPS = 2048, 12, 32, 3
    small = synth.env_cube(512, 1)[: 4 * 6 * 512 * 512].reshape(6, 512, 512, 4)
    big = np.repeat(np.repeat(small, 4, axis=1), 4, axis=2)
    yy, xx = np.meshgrid(np.arange(S, dtype=np.uint32), np.arange(S, dtype=np.uint32), indexing="ij")
    big[..., :3] *= (1.0 + 0.03 * (((xx * 7 + yy * 13) % 16).astype(np.float32) / 16.0))[None, :, :, None]
    chain = np.zeros(4 * cube_mip_offset(S, SM), dtype=np.float32)
    chain[: big.size] = big.reshape(-1)
    del big, small, xx, yy
    dsky = ctx.upload(chain)
    ctx.cube_gen_mips(dsky, S, SM)
    rng = np.random.default_rng(20480)
    for name, dev in (("half-representable", dsky.half().float()), ("fp32", dsky)):
        host = dev.cpu().numpy()
        got = to_np_half(ctx.prefilter_env(dev, S, SM, OUT, MIPS))
        ctx.sync()
        for m in range(MIPS):
            n = 6 * (OUT >> m) ** 2
            idx = np.sort(rng.choice(n, size=min(96, n), replace=False)).astype(np.uint32)
            want = orc.prefilter_env_texels(host, S, SM, OUT, MIPS, m, idx)
            sub = got[cube_mip_offset(OUT, m) + idx.astype(np.int64)]
            d = common.half_ulp_diff(sub[:, :3], want[:, :3])
            rel = np.abs(sub[:, :3].astype(np.float32) - want[:, :3].astype(np.float32)) <= 1e-3 * np.abs(want[:, :3].astype(np.float32))
            assert ((d <= 1) | rel).all(), (name, m, int(d.max()))


# ------------------------------------------------------------------------------------------ a14-a15
def _levels(flat, w, h):
    return [flat[bloom_level_offset(w, h, l): bloom_level_offset(w, h, l + 1)].reshape(h >> l, w >> l, 4) for l in range(5)]


def test_bloom_stages_bit_exact(ctx, orc):
    img = synth.hdr_noise_image(300, 170)       # odd half sizes: 150x85 -> 75x42 -> 37x21 -> 18x10
    d = dev_half(ctx, img)
    pre = ctx.zeros((85, 150, 4), torch.float16)
    ctx.bloom_prefilter(d, 300, 170, 300, pre)
    want_pre = orc.bloom_prefilter(img)
    assert np.array_equal(to_np_half(pre).view(np.uint16), want_pre.view(np.uint16))
    out = ctx.zeros((42, 75, 4), torch.float16)
    ctx.blur_h(pre, 150, 85, out, 75, 42)       # 2x downsample H
    want_h = orc.blur_h(want_pre, 75, 42)
    assert np.array_equal(to_np_half(out).view(np.uint16), want_h.view(np.uint16))
    out2 = ctx.zeros((42, 75, 4), torch.float16)
    ctx.blur_v(out, 75, 42, out2, 75, 42)
    want_v = orc.blur_v(want_h, 75, 42)
    assert np.array_equal(to_np_half(out2).view(np.uint16), want_v.view(np.uint16))
    up = ctx.zeros((85, 150, 4), torch.float16)
    ctx.bloom_upsample_add(pre, 150, 85, out2, 75, 42, up)
    want_up = orc.bloom_upsample_add(want_pre, want_v)
    assert np.array_equal(to_np_half(up).view(np.uint16), want_up.view(np.uint16))
    hdr = dev_half(ctx, img)
    big = dev_half(ctx, synth.hdr_noise_image(300, 170, seed=77))
    ctx.bloom_merge(hdr, 300, big, 300, 170)
    want_m = orc.bloom_merge(img.copy(), synth.hdr_noise_image(300, 170, seed=77))
    assert np.array_equal(to_np_half(hdr).view(np.uint16), want_m.view(np.uint16))


def test_blur_group_edges_wide_and_tall(ctx, orc):
    # > 256 texels in x and y: exercises the 256-group halo protocol of blur.hlsli:24-89 on both axes
    img = synth.hdr_noise_image(600, 530, seed=5)
    d = dev_half(ctx, img)
    o = ctx.zeros((530, 600, 4), torch.float16)
    ctx.blur_h(d, 600, 530, o, 600, 530)
    assert np.array_equal(to_np_half(o).view(np.uint16), orc.blur_h(img, 600, 530).view(np.uint16))
    ctx.blur_v(d, 600, 530, o, 600, 530)
    assert np.array_equal(to_np_half(o).view(np.uint16), orc.blur_v(img, 600, 530).view(np.uint16))


def test_bloom_chain_vs_golden_every_mip(ctx, orc, golden):
    """The reference's 16 dispatches issued one by one through the stage-level entry points (what the host pass graph
    does): every level of both chains equals the golden chain; pbr_bloom (which fuses level pairs where it can and
    treats the chains as scratch) gives the same HDR."""
    W, H = 128, 72
    img = synth.hdr_noise_image(W, H)
    hdr = dev_half(ctx, img)
    a, b = ctx.alloc_bloom_chain(W, H), ctx.alloc_bloom_chain(W, H)

    def lvl(t, l):   # device view of level l of a chain
        off = bloom_level_offset(W, H, l)
        return t.view(-1, 4)[off: off + (W >> l) * (H >> l)]

    dims = [(W >> l, H >> l) for l in range(5)]
    ctx.bloom_prefilter(hdr, W, H, W, lvl(a, 1))
    for i in range(3):                                   # downsample: H into chain B, V back into chain A
        up, lo = i + 1, i + 2
        ctx.blur_h(lvl(a, up), *dims[up], lvl(b, lo), *dims[lo])
        ctx.blur_v(lvl(b, lo), *dims[lo], lvl(a, lo), *dims[lo])
    for i in (2, 1, 0):                                  # upsample: V(H(lower) + H(upper))
        up = i + 1
        ctx.bloom_upsample_add(lvl(a, up), *dims[up], lvl(a, up + 1), *dims[up + 1], lvl(b, up))
        ctx.blur_v(lvl(b, up), *dims[up], lvl(a, up), *dims[up])
    ctx.blur_h(lvl(a, 1), *dims[1], lvl(b, 0), W, H)
    ctx.blur_v(lvl(b, 0), W, H, lvl(a, 0), W, H)
    ctx.bloom_merge(hdr, W, lvl(a, 0), W, H)
    ga, gb_ = to_np_half(a), to_np_half(b)
    for l in range(5):
        la, lb = _levels(ga, W, H)[l], _levels(gb_, W, H)[l]
        wa, wb = _levels(golden["bloom_chain_a"], W, H)[l], _levels(golden["bloom_chain_b"], W, H)[l]
        assert np.array_equal(la.view(np.uint16), wa.view(np.uint16)), f"chain A level {l}"
        assert np.array_equal(lb.view(np.uint16), wb.view(np.uint16)), f"chain B level {l}"
    assert np.array_equal(to_np_half(hdr).view(np.uint16), golden["bloom_hdr"].view(np.uint16))
    # pbr_bloom: 128x72 halves exactly three times (72, 36, 18, 9 | 4): fused kernels for those level pairs, staged ones
    # for 9 -> 4; same HDR
    hdr2 = dev_half(ctx, img)
    ctx.bloom(hdr2, W, H, W, ctx.alloc_bloom_chain(W, H), ctx.alloc_bloom_chain(W, H))
    assert np.array_equal(to_np_half(hdr2).view(np.uint16), golden["bloom_hdr"].view(np.uint16))


def test_bloom_histogram_fused_equals_separate(ctx, orc):
    # 300x170 (ragged tiles), histogram of an interior rectangle only (multi-GPU apron case)
    img = synth.hdr_noise_image(304, 176, seed=21)
    rect = (16, 32, 256, 112)
    hdr_a, hdr_b = dev_half(ctx, img), dev_half(ctx, img)
    ca, cb = ctx.alloc_bloom_chain(304, 176), ctx.alloc_bloom_chain(304, 176)
    hist_a = ctx.zeros((256,), torch.int32)
    ctx.bloom_histogram(hdr_a, 304, 176, 304, ca, cb, rect, hist_a)
    ctx.bloom(hdr_b, 304, 176, 304, ca, cb)
    got = to_np_half(hdr_a)
    assert np.array_equal(got.view(np.uint16), to_np_half(hdr_b).view(np.uint16))
    want_hdr = img.copy()
    orc.bloom(want_hdr)
    assert np.array_equal(got.view(np.uint16), want_hdr.view(np.uint16))
    x, y, w, h = rect
    want_hist = orc.lum_histogram(np.ascontiguousarray(want_hdr[y:y + h, x:x + w]))
    got_hist = hist_a.cpu().numpy().view(np.uint32)
    assert got_hist.sum() == w * h
    assert np.abs(got_hist.astype(np.int64) - want_hist.astype(np.int64)).sum() <= 2
    hist_b = ctx.zeros((256,), torch.int32)
    ctx.lum_histogram(hdr_b.data_ptr() + 8 * (y * 304 + x), w, h, 304, hist_b)
    assert np.array_equal(got_hist, hist_b.cpu().numpy().view(np.uint32))


def test_bloom_too_small_is_rejected(ctx):
    from direct12pbrrenderer_amd.api import PbrError
    hdr = ctx.zeros((8, 8, 4), torch.float16)
    with pytest.raises(PbrError):
        ctx.bloom(hdr, 8, 8, 8, ctx.alloc_bloom_chain(8, 8), ctx.alloc_bloom_chain(8, 8))


# ------------------------------------------------------------------------------------------ a16-a18
def test_histogram_average_tonemap_vs_golden(ctx, orc, golden):
    hdr_np = golden["bloom_hdr"]
    hdr = dev_half(ctx, hdr_np)
    hist = ctx.zeros((256,), torch.int32)
    ctx.lum_histogram(hdr, 128, 72, 128, hist)
    got_hist = hist.cpu().numpy().view(np.uint32)
    assert got_hist.sum() == 128 * 72
    assert np.abs(got_hist.astype(np.int64) - golden["hist"].astype(np.int64)).sum() <= 2   # boundary flips
    # average on the oracle's histogram: exact
    hist2 = ctx.upload(golden["hist"])
    avg = ctx.upload(np.array([0.18], dtype=np.float32))
    ctx.lum_average(hist2, 128 * 72, 1.0 / 60.0, avg)
    assert avg.cpu().numpy()[0] == pytest.approx(float(golden["avg"]), rel=2e-6)
    assert np.all(hist2.cpu().numpy() == 0)                         # cleared for the next frame
    ldr = ctx.zeros((72, 128), torch.int32)
    ctx.tonemap(hdr, 128, 72, 128, ctx.upload(np.array([golden["avg"]], dtype=np.float32)), ldr, 128)
    got = ldr.cpu().numpy().view(np.uint32)
    want = golden["ldr"]
    for k in range(4):
        dch = np.abs(((got >> (8 * k)) & 255).astype(np.int32) - ((want >> (8 * k)) & 255).astype(np.int32))
        assert dch.max() <= 1, f"channel {k}"
    assert np.all(got >> 24 == 255)


def test_histogram_ragged_and_accumulating(ctx, orc):
    img = synth.hdr_noise_image(333, 77, seed=9)                    # odd width: scalar path
    img[5, 5, :3] = 0.0                                             # a black pixel -> bin 0
    hist = ctx.zeros((256,), torch.int32)
    d = dev_half(ctx, img)
    ctx.lum_histogram(d, 333, 77, 333, hist)
    ctx.lum_histogram(d, 333, 77, 333, hist)                        # the pass ADDS (InterlockedAdd)
    want = orc.lum_histogram(img) * 2
    got = hist.cpu().numpy().view(np.uint32)
    assert got.sum() == want.sum() and got[0] == want[0] >= 2
    assert np.abs(got.astype(np.int64) - want.astype(np.int64)).sum() <= 4
    # interior view of a wider buffer (pitch > w, pointer offset)
    wide = np.zeros((77, 400, 4), dtype=np.float16)
    wide[:, 40:40 + 332] = img[:, :332]
    dw = dev_half(ctx, wide)
    hist.zero_()
    ctx.lum_histogram(dw.data_ptr() + 8 * 40, 332, 77, 400, hist)
    want2 = orc.lum_histogram(np.ascontiguousarray(img[:, :332]))
    assert np.abs(hist.cpu().numpy().view(np.uint32).astype(np.int64) - want2.astype(np.int64)).sum() <= 2


def test_average_truncation_overflow_and_black_frame(ctx, orc):
    def run(hist_np, count, dt, prev):
        h = ctx.upload(hist_np)
        a = ctx.upload(np.array([prev], dtype=np.float32))
        ctx.lum_average(h, count, dt, a)
        return a.cpu().numpy()[0]
    h = np.zeros(256, dtype=np.uint32)
    h[10], h[11] = 1, 3                                              # Q13 truncation
    assert run(h, 4, 1e9, 0.0) == np.float32(orc.lum_average(h.copy(), 4, 1e9, 0.0))
    h = np.zeros(256, dtype=np.uint32)
    h[255] = 20_000_000                                              # Q15 uint32 wrap
    assert run(h, 20_000_000, 1.0 / 60.0, 0.5) == pytest.approx(orc.lum_average(h.copy(), 20_000_000, 1.0 / 60.0, 0.5), rel=2e-6)
    h = np.zeros(256, dtype=np.uint32)
    h[0] = 100                                                       # Q14 all-black frame: 0/0
    got, want = run(h, 100, 1.0 / 60.0, 0.25), orc.lum_average(h.copy(), 100, 1.0 / 60.0, 0.25)
    assert (np.isnan(got) and np.isnan(want)) or got == pytest.approx(want, rel=2e-6)


def test_average_tonemap_one_launch_equals_the_two_dispatches(ctx, orc):
    """pbr_average_tonemap (round 4: every block of the tone-map re-derives the adapted luminance from the bins) against
    pbr_lum_average + pbr_tonemap: the same luminance cell and LDR image bit for bit, the OTHER histogram zeroed, the one read left
    alone; ragged and interior-view sizes; and the aliasing the contract forbids is refused."""
    from direct12pbrrenderer_amd.api import PbrError
    for (w, h, pitch, x0) in ((512, 288, 512, 0), (333, 77, 400, 40), (2, 2, 2, 0)):
        img = synth.hdr_noise_image(pitch, h, seed=w + h)
        d = dev_half(ctx, img)
        view = d.data_ptr() + 8 * x0
        hist = ctx.zeros((256,), torch.int32)
        ctx.lum_histogram(view, w, h, pitch, hist)
        hist_b, stale = hist.clone(), ctx.upload(np.arange(256, dtype=np.int32) + 7)
        for dt, prev in ((1.0 / 60.0, 0.18), (1e9, 0.0)):
            a = ctx.upload(np.array([prev], dtype=np.float32))
            h1 = hist.clone()
            ldr_a = ctx.zeros((h, w), torch.int32)
            ctx.lum_average(h1, w * h, dt, a)
            ctx.tonemap(view, w, h, pitch, a, ldr_a, w)
            a_in, a_out = ctx.upload(np.array([prev], dtype=np.float32)), ctx.upload(np.array([-1.0], dtype=np.float32))
            ldr_b = ctx.zeros((h, w), torch.int32)
            clear = stale.clone()
            ctx.average_tonemap(hist_b, w * h, dt, a_in, a_out, clear, view, w, h, pitch, ldr_b, w)
            ctx.sync()
            assert a_out.cpu().numpy().view(np.uint32)[0] == a.cpu().numpy().view(np.uint32)[0] and float(a_in.cpu()[0]) == np.float32(prev)
            assert torch.equal(ldr_a, ldr_b)
            assert int(clear.abs().sum()) == 0 and torch.equal(hist_b, hist) and int(h1.abs().sum()) == 0
    a = ctx.upload(np.array([0.18], dtype=np.float32))
    with pytest.raises(PbrError, match="avg_out must differ"):
        ctx.average_tonemap(hist, 4, 0.1, a, a, None, d, 2, 2, 2, ctx.zeros((2, 2), torch.int32), 2)
    with pytest.raises(PbrError, match="avg_out must differ"):
        ctx.average_tonemap(hist, 4, 0.1, a, a.clone(), hist, d, 2, 2, 2, ctx.zeros((2, 2), torch.int32), 2)


# ------------------------------------------------------------------------------------------ whole frame
def test_frame_1080p_region_properties_and_oracle_sample(ctx, orc, ibl):
    """cfg2-sized frame (1920x1080, 1 light): full-size run checked through size-independent
    properties plus an oracle comparison on a 96-row band."""
    from direct12pbrrenderer_amd.pipeline import DeferredFrame, TileSpec
    sky, env, lut, sh = ibl
    W, H = 1920, 1080
    cam, g, lights, gb, tile = common.shade_scene(W, H, 1, sh, rough_min=48, coverage_mask=False)
    spec = TileSpec(0, 0, W, H, W, H, 0)
    fr = DeferredFrame(ctx, spec, g, lights, dev_half(ctx, lut), lut.shape[0], dev_half(ctx, env), common.ENV_SIZE, common.ENV_MIPS)
    fr.upload_gbuffer(gb)
    fr.set_prev_luminance(0.18)
    fr.clustered()
    fr.shade()
    shaded = to_np_half(fr.hdr).copy()
    assert np.isfinite(shaded.astype(np.float32)).all()
    # oracle on a band of rows (global-pixel math makes a band == the same rows of the frame)
    y0, rows = 500, 96
    cl = orc.cluster_build(g)
    orc.cluster_cull(g, lights, cl)
    band = {k: np.ascontiguousarray(v[y0:y0 + rows]) for k, v in gb.items()}
    band_tile = Tile(0, y0, W, rows, W, H)
    want, want_f32 = orc.deferred_shade(g, band_tile, band, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights, want_f32=True)
    truth = _truth(orc, g, band_tile, band, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights)
    _check_shade(orc, shaded[y0:y0 + rows], want, want_f32, truth, band["stencil"], "1080p band", rough=band["C"] & 255)
    fr.bloom()
    fr.histogram()
    hist = fr.hist.cpu().numpy().view(np.uint32).copy()
    assert hist.sum() == W * H                                       # checksum of the histogram
    fr.average()
    fr.tonemap()
    ldr = fr.ldr_numpy()
    assert np.all(ldr >> 24 == 255)
    # tone-map is monotone in the exposed value: brighter HDR red never maps to a darker byte
    hdr_after = to_np_half(fr.hdr).astype(np.float32)
    r = hdr_after[..., 0].ravel()
    order = np.argsort(r, kind="stable")
    assert np.all(np.diff((ldr.ravel()[order] & 255).astype(np.int32)) >= 0)
    # bloom only adds light (weights and inputs are non-negative)
    assert np.all(hdr_after[..., :3] >= shaded.astype(np.float32)[..., :3] - 1e-3)


# ------------------------------------------------------------------------------------------ SURVEY 8f rows
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(64, 4), (333, 77), (1920, 1080)])
def test_gbuffer_encode_vs_oracle(ctx, orc, w, h):
    """gbuffer.hlsl::ps_main on per-pixel material planes: normals / roughness / metallic / AO / emission planes
    bit-exact; the gamma decode is exp2(2.2 log2 c) on the transcendental unit (what the shader compiler emits for
    pow; ~1e-6 relative vs libm powf), so albedo may differ by one 8-bit step on the ~1e-4 of the channel values
    that sit on a rounding boundary."""
    m0, m1, m2 = synth.material_tile(0, 0, w, h, w, h)
    wantA, wantB, wantC = orc.gbuffer_encode(m0, m1, m2)
    A, B, Cc = (ctx.zeros((h, w), torch.int32) for _ in range(3))
    ctx.gbuffer_encode(ctx.upload(m0), ctx.upload(m1), ctx.upload(m2), w, h, w, A, B, Cc)
    ctx.sync()
    A, B, Cc = (t.cpu().numpy().view(np.uint32) for t in (A, B, Cc))
    assert np.array_equal(B, wantB)
    assert np.array_equal(Cc, wantC)
    assert np.array_equal(A >> 24, wantA >> 24)
    da = np.abs(A.view(np.uint8).astype(np.int16) - wantA.view(np.uint8).astype(np.int16))
    assert da.max() <= 1 and (da > 0).mean() <= 3e-4, (da.max(), (da > 0).mean())


@pytest.mark.gpu
def test_gbuffer_encode_bad_args(ctx):
    from direct12pbrrenderer_amd.api import PbrError
    m = ctx.zeros((8, 8, 4), torch.float32)
    o = ctx.zeros((8, 8), torch.int32)
    with pytest.raises(PbrError, match="bad size"):
        ctx.gbuffer_encode(m, m, m, 8, 8, 4, o, o, o)
    with pytest.raises(PbrError, match="16-byte"):
        ctx.gbuffer_encode(m.view(-1)[1:], m, m, 4, 4, 4, o, o, o)


@pytest.mark.gpu
@pytest.mark.parametrize("sky_size,frame,tile", [(32, (320, 180), None), (256, (160, 90), None), (64, (640, 360), (328, 91, 200, 37))])
def test_skybox_vs_oracle(ctx, orc, sky_size, frame, tile):
    """skybox.hlsl on the stencil == 0 pixels: magnified (LOD 0), minified (trilinear, LOD ~2) and a ragged tile of
    a larger frame.  Same arithmetic as the oracle except log2f (device libm) -> a few texels differ by 1 half ULP."""
    W, H = frame
    x0, y0, w, h = tile if tile else (0, 0, W, H)
    mips = int(np.log2(sky_size)) + 1
    sky = synth.env_cube(sky_size)
    orc.cube_gen_mips(sky, sky_size, mips)
    cam = scene.Camera.reference_default(W, H)
    g = scene.make_global(cam, W, H)
    stencil = synth.gbuffer_tile(x0, y0, w, h, W, H, coverage_mask=True)["stencil"]
    stencil[:, : w // 3] = 0                                           # a large sky region + the 16x16 holes
    t = Tile(x0, y0, w, h, W, H)
    want = np.full((h, w, 4), 3.0, np.float16)
    orc.skybox(g, t, sky, sky_size, mips, stencil, want)
    hdr = dev_half(ctx, np.full((h, w, 4), 3.0, np.float16))
    ctx.skybox(g, t, ctx.upload(sky), sky_size, mips, ctx.upload(stencil), w, hdr, w)
    ctx.sync()
    got = to_np_half(hdr)
    off = stencil == 0
    assert off.sum() > w * h // 4
    assert np.all(got[~off] == 3.0)                                    # geometry pixels untouched
    d = common.half_ulp_diff(got[off], want[off])
    assert d.max() <= 2 and (d > 0).mean() <= 2e-3, (d.max(), (d > 0).mean())


@pytest.mark.gpu
def test_skybox_then_shade_compose(ctx, orc, ibl):
    """SkyboxPass then DeferredShadingPass on one target: each pass owns its half of the stencil partition."""
    sky, env, lut, sh = ibl
    cam, g, lights, gb, tile = common.shade_scene(320, 192, 256, sh, rough_min=48, coverage_mask=True)
    cl = orc.cluster_build(g)
    orc.cluster_cull(g, lights, cl)
    want, _ = orc.deferred_shade(g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights)
    orc.skybox(g, tile, sky, common.SKY_SIZE, common.SKY_MIPS, gb["stencil"], want)
    from direct12pbrrenderer_amd.pipeline import DeferredFrame, TileSpec
    fr = DeferredFrame(ctx, TileSpec(0, 0, 320, 192, 320, 192, 0), g, lights, dev_half(ctx, lut),
                       common.LUT_RES, dev_half(ctx, env), common.ENV_SIZE, common.ENV_MIPS,
                       sky=(ctx.upload(sky), common.SKY_SIZE, common.SKY_MIPS))
    fr.upload_gbuffer(gb)
    fr.clustered()
    fr.skybox()
    fr.shade()
    ctx.sync()
    got = to_np_half(fr.hdr)
    off = gb["stencil"] == 0
    assert off.sum() > 1000 and (~off).sum() > 1000
    d_sky = common.half_ulp_diff(got[off], want[off])
    assert d_sky.max() <= 2
    d = common.half_ulp_diff(got[~off][:, :3], want[~off][:, :3])
    assert (d > 2).mean() <= 1e-3


@pytest.mark.gpu
def test_rgbe_decode_bit_exact(ctx, orc):
    """Radiance RGBE -> fp32: every exponent byte (incl. 0 and the subnormal scales below e = 10) x random mantissas,
    plus a ragged count; exact (power-of-two scale)."""
    rng = np.random.default_rng(0x5EED0040)
    n = 256 * 257 + 13
    t = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    t[:256 * 257, 3] = np.repeat(np.arange(256, dtype=np.uint8), 257)
    want = orc.rgbe_decode(t)
    out = ctx.zeros((n, 4), torch.float32)
    ctx.rgbe_decode(torch.from_numpy(t).to(ctx.torch_device), out)
    ctx.sync()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert (want[t[:, 3] == 0][:, :3] == 0).all() and (want[:, 3] == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(2048, 64), (1040, 48), (512, 288), (304, 176), (320, 180), (480, 270), (400, 300), (360, 192)])
def test_bloom_fused_exact_pyramid_bit_exact(ctx, orc, w, h):
    """(320x180: heights 180, 90, 45, 22, 11 — exact, exact, NOT exact, exact: fused and staged kernels alternate per
    level pair; 480x270 = 1080p / 4: heights 270, 135, 67, 33, 16 — only the first pair is exact; 400x300: heights 300, 150,
    75, 37, 18 — two exact pairs then two staged ones; 360x192: the WIDTH stops halving exactly at 45 -> 22.)
    Exact 2x pyramids take the fused path (shared-sample prefilter; H+V of a level in one kernel with the H
    result kept in registers; merge + histogram in the last one): final HDR bit-identical to the oracle's staged
    chain, histogram equal to the stand-alone pass.  Sizes cover 256- and 64-column blocks, ragged widths/heights."""
    img = synth.hdr_noise_image(w, h, seed=w + h)
    want = img.copy()
    orc.bloom(want)
    hdr = dev_half(ctx, img)
    ca, cb = ctx.alloc_bloom_chain(w, h), ctx.alloc_bloom_chain(w, h)
    hist = ctx.zeros((256,), torch.int32)
    ctx.bloom_histogram(hdr, w, h, w, ca, cb, (0, 0, w, h), hist)
    got = to_np_half(hdr)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    # the shared-sample prefilter on its own (chain contents after pbr_bloom are scratch)
    pf = ctx.zeros((h // 2, w // 2, 4), torch.float16)
    ctx.bloom_prefilter(dev_half(ctx, img), w, h, w, pf)
    assert np.array_equal(to_np_half(pf).view(np.uint16), orc.bloom_prefilter(img).view(np.uint16))
    hist_ref = ctx.zeros((256,), torch.int32)
    ctx.lum_histogram(hdr, w, h, w, hist_ref)
    assert np.array_equal(hist.cpu().numpy(), hist_ref.cpu().numpy())
    # without the histogram
    hdr2 = dev_half(ctx, img)
    ctx.bloom(hdr2, w, h, w, ca, cb)
    assert np.array_equal(to_np_half(hdr2).view(np.uint16), want.view(np.uint16))


_WIDE_BLOOM = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
from oracle import binding as orc
from direct12pbrrenderer_amd import synth
from direct12pbrrenderer_amd.api import PbrContext
import common
EXACT = %r
ctx = PbrContext(0)
up = lambda a: ctx.upload(np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)).view(torch.float16)
down = lambda t: t.cpu().view(torch.int16).numpy().view(np.float16)
def same(got, want, what):
    # EXACT: the shader-order kernels, bit for bit.  Otherwise the polyphase 2x-up kernel ran somewhere in the chain: every texel
    # within 2 fp16 ULP of the oracle's staged chain end to end, and all but a sliver identical
    if EXACT:
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), (what, int((got.view(np.uint16) != want.view(np.uint16)).sum()))
    else:
        d = common.half_ulp_diff(got[..., :3], want[..., :3])
        assert d.max() <= 2 and (d > 0).mean() <= 2e-3 and (d > 1).mean() <= 1e-4, (what, int(d.max()), float((d > 0).mean()), float((d > 1).mean()))
for (w, h) in %r:
    img = synth.hdr_noise_image(w, h, seed=w + h)
    want = img.copy()
    orc.bloom(want)
    ca, cb = ctx.alloc_bloom_chain(w, h), ctx.alloc_bloom_chain(w, h)
    hdr, hist = up(img), ctx.zeros((256,), torch.int32)
    ctx.bloom_histogram(hdr, w, h, w, ca, cb, (0, 0, w, h), hist)
    got = down(hdr)
    same(got, want, ("bloom+histogram", w, h))
    ref = ctx.zeros((256,), torch.int32)
    ctx.lum_histogram(hdr, w, h, w, ref)
    assert np.array_equal(hist.cpu().numpy(), ref.cpu().numpy()), ("histogram", w, h)
    hdr2 = up(img)
    ctx.bloom(hdr2, w, h, w, ca, cb)
    assert np.array_equal(down(hdr2).view(np.uint16), got.view(np.uint16)), ("bloom without histogram = bloom with", w, h)
    # a histogram rectangle that is not the frame
    hdr3, hist3, ref3 = up(img), ctx.zeros((256,), torch.int32), ctx.zeros((256,), torch.int32)
    rect = (w // 8, h // 16, w // 2 + 3, h // 2 + 1)
    ctx.bloom_histogram(hdr3, w, h, w, ca, cb, rect, hist3)
    ctx.sync()
    sub = down(hdr3)[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]
    ctx.lum_histogram(up(sub), rect[2], rect[3], rect[2], ref3)
    assert np.array_equal(hist3.cpu().numpy(), ref3.cpu().numpy()), ("histogram rect", w, h)
    # ONE upsample level as a stage (pbr_bloom_up_level) on the oracle's own inputs: <= 1 fp16 ULP (EXACT: 0) from the two staged dispatches
    if w %% 4 == 0 and h %% 4 == 0:
        lower = synth.hdr_noise_image(w // 2, h // 2, seed=3 * w + h)
        for upper in (synth.hdr_noise_image(w, h, seed=w + 7 * h), None):
            out = ctx.zeros((h, w, 4), torch.float16)
            ctx.bloom_up_level(up(upper) if upper is not None else None, up(lower), w // 2, h // 2, out, w, h)
            b = orc.bloom_upsample_add(upper, lower) if upper is not None else orc.blur_h(lower, w, h)
            want_l = orc.blur_v(b, w, h)
            d = common.half_ulp_diff(down(out), want_l)
            assert d.max() <= (0 if EXACT else 1) and (d > 0).mean() <= 1e-3, ("up level", w, h, upper is not None, int(d.max()), float((d > 0).mean()))
ctx.close()
print("wide bloom ok")
"""


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("knobs,exact,sizes", [   # ids as before a fourth row (knobs1) was retired, so that each id keeps naming the same case
    pytest.param({"PBR_BLOOM_WIDE": "1"}, False, [(2048, 64), (1040, 48), (512, 288), (304, 176), (320, 180), (96, 32), (400, 304), (160, 2080)],
                 id="knobs0-False-sizes0"),
    pytest.param({"PBR_BLOOM_WIDE": "0"}, True, [(512, 288), (2080, 1296)], id="knobs2-True-sizes2"),
    pytest.param({}, False, [(2080, 1296), (3328, 2048)], id="knobs3-False-sizes3"),
])
def test_bloom_2x_up_levels_polyphase_and_shader_order(knobs, exact, sizes):
    """The 2x-up levels of the bloom pyramid against the oracle's staged chain.  Large levels (>= 400 tiles of 128 x 32) run
    k_blur_up_poly, the polyphase form (two six-tap filters on the coarse row, then the 1/4 | 3/4 row blend): held to SURVEY 8c's
    bloom-stage tolerance — each level as a stage (pbr_bloom_up_level, on the oracle's own inputs) <= 1 fp16 ULP, the whole chain
    <= 2 ULP end to end with >= 99.8 % of the texels identical — where round 3 demanded bit-exactness.  The bit-exact checker is k_blur_hv,
    the shader-order kernel (knobs build, PBR_BLOOM_WIDE=0): bit for bit.
    Forced on at small and ragged sizes every M_UP level of the pyramid runs the polyphase kernel: widths below one tile, widths that
    are no multiple of 128, a 5-texel-wide level, image edges inside the first and last rows of waves.  Product library, chosen by
    the threshold — 2080x1296: the final level only; 3328x2048: level 1 (DUAL instance) as well.  The switches are read once per
    process and exist in the knobs build only (the product library never reads the environment), hence the child process."""
    import os
    root = common.ROOT
    r = common.run_child(_WIDE_BLOOM % (root, os.path.join(root, "tests"), exact, sizes), knobs, clear=("PBR_BLOOM_WIDE",), timeout_s=800)
    assert r.returncode == 0 and "wide bloom ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.gpu
def test_bloom_shader_order_switch_is_bit_exact_at_large_sizes(ctx, orc):
    """pbr_ctx_set_bloom_shader_order (PRODUCT library): with the switch on the two large 2x-up levels run the shader-order
    kernels instead of the polyphase form, and a frame above the ~1.6 Mpixel threshold is bit-identical to the oracle's staged chain —
    what a host needs that compares a rank's tile with the whole frame; off again, the same call is within 2 fp16 ULP."""
    w, h = 2080, 1296          # the merge level takes the polyphase kernel by default (650 tiles of 128 x 32)
    img = synth.hdr_noise_image(w, h, seed=w + h)
    want = img.copy()
    orc.bloom(want)
    up = lambda a: ctx.upload(np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)).view(torch.float16)   # noqa: E731
    ca, cb = ctx.alloc_bloom_chain(w, h), ctx.alloc_bloom_chain(w, h)
    try:
        ctx.set_bloom_shader_order(True)
        hdr, hist = up(img), ctx.zeros((256,), torch.int32)
        ctx.bloom_histogram(hdr, w, h, w, ca, cb, (0, 0, w, h), hist)
        ctx.sync()
        got = hdr.cpu().view(torch.int16).numpy().view(np.float16)
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), int((got.view(np.uint16) != want.view(np.uint16)).sum())
        assert int(hist.sum()) == w * h
    finally:
        ctx.set_bloom_shader_order(False)
    hdr2 = up(img)
    ctx.bloom(hdr2, w, h, w, ca, cb)
    ctx.sync()
    d = common.half_ulp_diff(hdr2.cpu().view(torch.int16).numpy().view(np.float16)[..., :3], want[..., :3])
    assert 0 < d.max() <= 2          # the default path is the polyphase one here: close, not identical


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160)])
def test_bloom_up_levels_scale_exactly_at_full_size(ctx, w, h):
    """A size-independent property of the two large 2x-up levels of the 4K frame, without the CPU: the upsample, the two six-tap
    polyphase filters, the nine same-size taps and the V pass are LINEAR, every intermediate is rounded to fp16 where a dispatch stores
    it, and scaling by a power of two commutes with every one of those roundings (no overflow, no subnormals on this input) — so doubling
    both inputs must double every output texel BIT FOR BIT.  1920x1080 = level 1 of the 4K pyramid (k_blur_up_poly, DUAL instance, 510
    tiles); 3840x2160 = the merge level's blur (the instance without the merge, 2 040 tiles).  A tap with a wrong weight, a halo entry from
    the wrong column, a tile seam or a row blend off by one survive no such test: every output would still be 'plausible'."""
    lower = synth.hdr_noise_image(w // 2, h // 2, seed=3 * w + h, impulse=False)
    upper = synth.hdr_noise_image(w, h, seed=w + 7 * h, impulse=False)
    up = lambda a: ctx.upload(np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)).view(torch.float16)   # noqa: E731
    lo1, up1 = up(lower), up(upper)
    lo2, up2 = lo1 * 2, up1 * 2                      # exact in fp16 (values in [2^-6, 2^3])
    for dual in (True, False):
        o1, o2 = ctx.zeros((h, w, 4), torch.float16), ctx.zeros((h, w, 4), torch.float16)
        ctx.bloom_up_level(up1 if dual else None, lo1, w // 2, h // 2, o1, w, h)
        ctx.bloom_up_level(up2 if dual else None, lo2, w // 2, h // 2, o2, w, h)
        ctx.sync()
        assert bool(torch.isfinite(o1).all()) and float(o1[..., :3].min()) > 2.0 ** -13      # no subnormal anywhere near
        assert bool(torch.equal(o2[..., :3], o1[..., :3] * 2)), (w, h, dual, int((o2[..., :3] != o1[..., :3] * 2).sum()))
        # ... and the level is not trivially zero or a copy: it is a blur (smaller spread than its input, same mean to 1 %)
        m_in = (up1[..., :3].float().mean() if dual else 0.0) + lo1[..., :3].float().mean()
        assert abs(float(o1[..., :3].float().mean()) / float(m_in) / (0.9999 ** 2) - 1.0) < 0.01


@pytest.mark.gpu
def test_bloom_4k_constant_field_is_uniform_and_size_independent(ctx, orc):
    """A size-independent property at BASELINE's full size (3840x2160: both polyphase instances run, 2 040 + 510 tiles): a constant HDR
    field stays constant through every level (clamp addressing, weights summing to 0.9999 per pass), so the bloomed frame is ONE value
    everywhere — borders, tile seams, the partial bottom tiles — and that value is the one the oracle computes on a small constant
    image (<= 1 fp16 ULP: the polyphase levels; the small image takes the shader-order kernels)."""
    W, H = 3840, 2160
    for rgb in ((2.0, 1.5, 0.75), (6.0, 0.5, 0.25)):
        small = np.zeros((72, 128, 4), np.float16)
        small[..., :3] = rgb
        small[..., 3] = 1.0
        want = small.copy()
        orc.bloom(want)
        assert (want.reshape(-1, 4) == want[0, 0]).all()          # the oracle agrees that the field stays constant
        img = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
        img[..., 0], img[..., 1], img[..., 2], img[..., 3] = rgb[0], rgb[1], rgb[2], 1.0
        hist = ctx.zeros((256,), torch.int32)
        ctx.bloom_histogram(img, W, H, W, ctx.alloc_bloom_chain(W, H), ctx.alloc_bloom_chain(W, H), (0, 0, W, H), hist)
        ctx.sync()
        flat = img.view(-1, 4)
        assert bool((flat == flat[0]).all()), "the bloomed constant field is not uniform"
        got = flat[0].cpu().view(torch.int16).numpy().view(np.float16)
        assert common.half_ulp_diff(got[:3], want[0, 0, :3]).max() <= 1, (got, want[0, 0])
        assert int(hist.sum()) == W * H and int((hist > 0).sum()) == 1    # one luminance, one bin


@pytest.mark.gpu
def test_deferred_shade_attenuation_floor_and_odd_lists(ctx, orc, ibl):
    """Lights whose attenuation polynomial can drop below the shader's 1e-6 floor (C0 = 0: the floor binds near the
    light) take the kernel's unhoisted-floor path; 7 lights give odd per-cluster lists (padded with the null light)."""
    sky, env, lut, sh = ibl
    cam, g, lights, gb, tile = common.shade_scene(256, 144, 256, sh, rough_min=48)
    lights = lights[:7].copy()
    lights["C0"][::2] = 0.0
    lights["C1"][::2] = 0.0
    lights["C2"][::2] = 1e-9
    lights["Intensity"][::2] = 1e-7          # keeps the radiance finite where 1/max(Q, 1e-6) = 1e6
    cl = orc.cluster_build(g)
    orc.cluster_cull(g, lights, cl)
    assert (cl["NumLights"] % 2 == 1).any()
    want, want_f32 = orc.deferred_shade(g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights, want_f32=True)
    truth = _truth(orc, g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights)
    got = _shade_on_gpu(ctx, g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights)
    _check_shade(orc, got, want, want_f32, truth, gb["stencil"], "attenuation floor / odd lists", rough=gb["C"] & 255)


@pytest.mark.gpu
@pytest.mark.parametrize("n_lights", [0, 5, 256, 1024])
def test_clustered_single_launch_equals_build_then_cull(ctx, ibl, n_lights):
    sky, env, lut, sh = ibl
    cam = scene.Camera.reference_default(1280, 720)
    g = scene.make_global(cam, 1280, 720, sh_pack=sh)
    lights = synth.lights_in_view_box(max(n_lights, 1), cam)[:n_lights]
    dl = ctx.upload(lights) if n_lights else None
    a, b = ctx.alloc_clusters(), ctx.alloc_clusters()
    a.fill_(0x55)                       # stale contents must not leak into the single-launch result
    ctx.clustered(g, dl, n_lights, a)
    ctx.cluster_build(g, b)
    ctx.cluster_cull(g, dl, n_lights, b)
    ctx.sync()
    ca = np.frombuffer(a.cpu().numpy().tobytes(), dtype=CLUSTER_DTYPE)
    cb = np.frombuffer(b.cpu().numpy().tobytes(), dtype=CLUSTER_DTYPE)
    assert np.array_equal(ca["MinBound"].view(np.uint32), cb["MinBound"].view(np.uint32))
    assert np.array_equal(ca["MaxBound"].view(np.uint32), cb["MaxBound"].view(np.uint32))
    assert np.array_equal(ca["NumLights"], cb["NumLights"])
    for k in range(32):
        used = ca["NumLights"] > k
        assert np.array_equal(ca["LightIndex"][used, k], cb["LightIndex"][used, k])


@pytest.mark.gpu
def test_frame_4k_256_lights_full_size_properties_tiles_and_oracle_band(ctx, orc, ibl):
    """BASELINE cfg4 size (3840x2160, 256 clustered lights + IBL) through the frame's own entry points (fused bloom,
    histogram in the bloom tail): an oracle comparison on a 64-row band of the shade, size-independent properties of the
    whole frame, and the cfg5 construction at full tile size — the frame cut into two 1920x2160 tiles with a 256-px
    apron reproduces the single-frame interior (HDR to <= 2 fp16 ulp, identical summed histogram up to boundary flips)."""
    from direct12pbrrenderer_amd.pipeline import DeferredFrame, TileSpec
    sky, env, lut, sh = ibl
    W, H = 3840, 2160
    cam, g, lights, gb, tile = common.shade_scene(W, H, 256, sh, rough_min=48, coverage_mask=False)
    dlut, denv = dev_half(ctx, lut), dev_half(ctx, env)

    def frame(spec):
        fr = DeferredFrame(ctx, spec, g, lights, dlut, lut.shape[0], denv, common.ENV_SIZE, common.ENV_MIPS)
        fr.upload_gbuffer({k: np.ascontiguousarray(v[spec.ey0:spec.ey1, spec.ex0:spec.ex1]) for k, v in gb.items()})
        fr.set_prev_luminance(0.18)
        return fr

    full = frame(TileSpec(0, 0, W, H, W, H, 0))
    full.clustered()
    full.shade()
    shaded = to_np_half(full.hdr).copy()
    assert np.isfinite(shaded.astype(np.float32)).all()
    y0, rows = 1040, 64
    cl = orc.cluster_build(g)
    orc.cluster_cull(g, lights, cl)
    band = {k: np.ascontiguousarray(v[y0:y0 + rows]) for k, v in gb.items()}
    band_tile = Tile(0, y0, W, rows, W, H)
    want, want_f32 = orc.deferred_shade(g, band_tile, band, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights, want_f32=True)
    truth = _truth(orc, g, band_tile, band, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights)
    _check_shade(orc, shaded[y0:y0 + rows], want, want_f32, truth, band["stencil"], "4K band", hard_ulp=None, rough=band["C"] & 255)
    full.bloom_histogram()
    hist_full = full.hist.cpu().numpy().view(np.uint32).copy()
    assert hist_full.sum() == W * H
    full.average()
    full.tonemap()
    hdr_full = to_np_half(full.hdr)
    assert np.all(hdr_full.astype(np.float32)[..., :3] >= shaded.astype(np.float32)[..., :3] - 1e-3)   # bloom only adds light
    assert np.all(full.ldr_numpy() >> 24 == 255)
    # two tiles + apron
    hist_sum = np.zeros(256, np.int64)
    for x0 in (0, 1920):
        spec = TileSpec(x0, 0, 1920, H, W, H, 256)
        assert (spec.ew, spec.eh) == (1920 + 256, H)
        t = frame(spec)
        t.clustered()
        t.shade()
        t.bloom_histogram()
        hist_sum += t.hist.cpu().numpy().view(np.uint32)
        got = to_np_half(t.hdr)[:, spec.ix:spec.ix + 1920]
        d = common.half_ulp_diff(got[..., :3], hdr_full[:, x0:x0 + 1920, :3])
        assert d.max() <= 2, (x0, d.max())
    assert hist_sum.sum() == W * H and np.abs(hist_sum - hist_full.astype(np.int64)).sum() <= 64


@pytest.mark.gpu
def test_frame_4k_halo_tiles_full_size_vs_single_frame(ctx, ibl):
    """The multi-GPU halo path at full tile size on one GPU (the big-tile kernel variants, 2x2 layout with corners):
    the 4K frame as four 1920x1080-ish tiles is not 16-aligned, so 3840x2176 is cut 2x2 into 1920x1088 tiles.  Every tile
    shades interior + 4 px, prefilters its interior, the level-1 strips travel by device-to-device copies driven by
    halo_plan (what pbr_halo_exchange does over RCCL), then pbr_bloom_tiled; interiors must equal the single-frame
    render to <= 2 fp16 ulp and the four histograms must add up to the frame's."""
    from direct12pbrrenderer_amd.pipeline import DeferredFrame, HaloTransport, TileSpec, tile_of_frame
    sky, env, lut, sh = ibl
    W, H = 3840, 2176
    cam, g, lights, gb, _ = common.shade_scene(W, H, 256, sh, rough_min=48, coverage_mask=False)
    dlut, denv = dev_half(ctx, lut), dev_half(ctx, env)

    class Manual(HaloTransport):
        def __init__(self):
            self.kind = "manual"

        def exchange(self, fr):
            pass

    def make(spec, specs=None, rank=0):
        fr = DeferredFrame(ctx, spec, g, lights, dlut, lut.shape[0], denv, common.ENV_SIZE, common.ENV_MIPS,
                           all_specs=specs, rank=rank, halo_transport=Manual() if spec.halo else None)
        fr.upload_gbuffer({k: np.ascontiguousarray(v[spec.sy0:spec.sy1, spec.sx0:spec.sx1]) for k, v in gb.items()})
        return fr

    full = make(TileSpec(0, 0, W, H, W, H, 0))
    full.clustered(); full.shade(); full.bloom_histogram()
    hdr_full = to_np_half(full.hdr)
    hist_full = full.hist.cpu().numpy().view(np.uint32).astype(np.int64)
    del full
    specs = [tile_of_frame(r, 4, W, H, layout=(2, 2), halo=True) for r in range(4)]
    assert (specs[3].sx0, specs[3].sy0, specs[3].sw, specs[3].sh) == (1916, 1084, 1924, 1092) and specs[0].ew == 1920 + 256
    tiles = [make(s, specs, r) for r, s in enumerate(specs)]
    for t in tiles:
        t.level1.fill_(777.0)
        t.clustered(); t.shade(); t.halo_prefilter()
    planes = [t.level1.view(t.spec.eh // 2, t.spec.ew // 2, 4) for t in tiles]
    for r, t in enumerate(tiles):                      # what r receives from n is n's send rectangle towards r
        for n, snd, rcv in t.halo_plan_local:
            if rcv is None:
                continue
            back = [q for q in tiles[n].halo_plan_local if q[0] == r][0][1]
            assert back is not None and (back[2], back[3]) == (rcv[2], rcv[3])
            planes[r][rcv[1]:rcv[1] + rcv[3], rcv[0]:rcv[0] + rcv[2]] = planes[n][back[1]:back[1] + back[3], back[0]:back[0] + back[2]]
    hist_sum = np.zeros(256, np.int64)
    for t in tiles:
        assert not bool((t.level1 == 777.0).any())
        t.halo_pyramid(histogram=True)
        s = t.spec
        d = common.half_ulp_diff(t.hdr_interior()[..., :3], hdr_full[s.y0:s.y0 + s.h, s.x0:s.x0 + s.w, :3])
        assert d.max() <= 2 and (d > 0).mean() < 2e-3, (s.x0, s.y0, d.max(), (d > 0).mean())
        hist_sum += t.hist.cpu().numpy().view(np.uint32)
    assert hist_sum.sum() == W * H and np.abs(hist_sum - hist_full).sum() <= 64


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_frame_8k_cfg5_full_size_band_properties_and_tiles(ctx, orc, ibl):
    """BASELINE cfg5 at its real size on one GPU: the 7680x4320 frame (256 clustered lights + IBL) — an oracle band of the
    shade, size-independent properties of the whole frame, and ONE rank's 1920x2160 tile of the 2 rows x 4 cols layout
    (rank 1: neighbours on three sides + two corners) in both border modes against the single-frame interior: apron mode
    as it runs on a GPU of the node, halo mode with the level-1 strips taken from the full frame's own level 1 (what the
    five neighbours would send: every level-1 texel is computed once, by its owner, from identical pixels)."""
    from direct12pbrrenderer_amd.pipeline import DeferredFrame, HaloTransport, TileSpec, parse_layout, tile_of_frame
    from direct12pbrrenderer_amd.structs import bloom_level_offset
    sky, env, lut, sh = ibl
    W, H = 7680, 4320
    cam, g, lights, gb, _ = common.shade_scene(W, H, 256, sh, rough_min=48, coverage_mask=False)
    dlut, denv = dev_half(ctx, lut), dev_half(ctx, env)

    class Manual(HaloTransport):
        def __init__(self):
            self.kind = "manual"

        def exchange(self, fr):
            pass

    def make(spec, specs=None, rank=0):
        fr = DeferredFrame(ctx, spec, g, lights, dlut, lut.shape[0], denv, common.ENV_SIZE, common.ENV_MIPS,
                           all_specs=specs, rank=rank, halo_transport=Manual() if spec.halo else None)
        fr.upload_gbuffer({k: np.ascontiguousarray(v[spec.sy0:spec.sy1, spec.sx0:spec.sx1]) for k, v in gb.items()})
        return fr

    full = make(TileSpec(0, 0, W, H, W, H, 0))
    full.clustered(); full.shade()
    shaded = to_np_half(full.hdr)
    assert np.isfinite(shaded.astype(np.float32)).all()
    y0, rows = 2128, 32
    cl = orc.cluster_build(g)
    orc.cluster_cull(g, lights, cl)
    band = {k: np.ascontiguousarray(v[y0:y0 + rows]) for k, v in gb.items()}
    band_tile = Tile(0, y0, W, rows, W, H)
    want, want_f32 = orc.deferred_shade(g, band_tile, band, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights, want_f32=True)
    truth = _truth(orc, g, band_tile, band, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights)
    _check_shade(orc, shaded[y0:y0 + rows], want, want_f32, truth, band["stencil"], "8K band", hard_ulp=None, rough=band["C"] & 255)
    # the full frame's level 1 (prefilter of the shaded frame), before bloom overwrites the chains
    l1_full = ctx.zeros((H // 2, W // 2, 4), torch.float16)
    ctx.bloom_prefilter(full.hdr, W, H, W, l1_full)
    full.bloom_histogram()
    hist_full = full.hist.cpu().numpy().view(np.uint32)
    assert hist_full.sum() == W * H
    hdr_full = to_np_half(full.hdr)
    assert np.all(hdr_full.astype(np.float32)[..., :3] >= shaded.astype(np.float32)[..., :3] - 1e-3)   # bloom only adds light
    del full, shaded
    lay = parse_layout("2x4")
    for halo in (False, True):
        specs = [tile_of_frame(r, 8, W, H, layout=lay, halo=halo) for r in range(8)]
        s = specs[1]
        assert (s.x0, s.y0, s.w, s.h, s.ew, s.eh) == (1920, 0, 1920, 2160, 2432, 2416)
        t = make(s, specs, 1)
        t.clustered(); t.shade()
        if halo:
            t.halo_prefilter()
            plane = t.level1.view(s.eh // 2, s.ew // 2, 4)
            own = plane[s.iy // 2:(s.iy + s.h) // 2, s.ix // 2:(s.ix + s.w) // 2].clone()
            plane.copy_(l1_full[s.ey0 // 2:s.ey1 // 2, s.ex0 // 2:s.ex1 // 2])          # the neighbours' strips ...
            assert torch.equal(plane[s.iy // 2:(s.iy + s.h) // 2, s.ix // 2:(s.ix + s.w) // 2], own)   # ... and the owner's texels agree bit for bit
            t.halo_pyramid(histogram=True)
        else:
            t.bloom_histogram()
        d = common.half_ulp_diff(t.hdr_interior()[..., :3], hdr_full[s.y0:s.y0 + s.h, s.x0:s.x0 + s.w, :3])
        assert d.max() <= 2 and (d > 0).mean() < 2e-3, (halo, d.max(), (d > 0).mean())
        assert t.hist.cpu().numpy().view(np.uint32).sum() == s.w * s.h
        del t


_SHADE_SCHEDULE = r"""
import hashlib, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import common
from direct12pbrrenderer_amd.api import PbrContext
from oracle import binding as orc
ctx = PbrContext(0)
sky, env, lut, sh = common.small_ibl(orc)
up = lambda a: ctx.upload(np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)).view(torch.float16)
lut_d, env_d = up(lut), ctx.env_pad(up(env), common.ENV_SIZE, common.ENV_MIPS)
out = []
for (w, h, full, x0, y0, n) in %r:
    cam, g, lights, gb, tile = common.shade_scene(w, h, n, sh, full=full, x0=x0, y0=y0)
    cl = orc.cluster_build(g); orc.cluster_cull(g, lights, cl)
    gbd = {k: ctx.upload(v) for k, v in gb.items()}
    hdr = ctx.zeros((h, w, 4), torch.float16)
    ctx.deferred_shade(g, tile, gbd, w, lut_d, lut.shape[0], env_d, common.ENV_SIZE, common.ENV_MIPS, ctx.upload(cl), ctx.upload(lights) if n else None, n, hdr, w)
    ctx.sync()
    got = hdr.cpu().view(torch.int16).numpy()
    line = hashlib.sha1(got.tobytes()).hexdigest()
    if %r:   # the oracle on the same inputs (stencil-masked pixels keep the zeros of the buffer on both sides)
        want, _ = orc.deferred_shade(g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights)
        d = common.half_ulp_diff(got.view(np.float16)[..., :3], want[..., :3])
        assert (d > 2).mean() <= 1e-3 and np.isfinite(got.view(np.float16).astype(np.float32)).all(), (w, h, int(d.max()), float((d > 2).mean()))
    out.append(line)
print("shade schedule", " ".join(out))
"""


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_deferred_shade_output_does_not_depend_on_the_launch_schedule():
    """Round 6: the shade sizes its blocks by the render target (rows per long block: 8 where that makes >= 1.3 generations of resident
    blocks, 2 .. 7 below — shade.hip, shade_schedule).  Per-pixel arithmetic must not know: the same frames shaded by the product library
    (rows by rule) and by the knobs build with every row count forced (PBR_SHADE_ROWS_BIG = 1 .. 8, and another two-zone split) are
    bit-identical — odd sizes (last block row / column partial), a tile of a larger frame (global pixel coordinates), 0 / 1 / 256 lights;
    and the product's frames agree with the oracle.  Own processes: the knobs are read once per process."""
    import os
    root = common.ROOT
    cases = [(321, 187, None, 0, 0, 256), (1441, 97, None, 0, 0, 256), (257, 64, (1440, 960), 1100, 850, 256), (640, 360, None, 0, 0, 1), (96, 33, None, 0, 0, 0)]

    def run(env_extra, check):
        r = common.run_child(_SHADE_SCHEDULE % (root, os.path.join(root, "tests"), cases, check), env_extra,
                             clear=("PBR_SHADE_ROWS_BIG", "PBR_SHADE_ROWS_SMALL", "PBR_SHADE_BIGFRAC"), timeout_s=600)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("shade schedule")]
        assert r.returncode == 0 and lines, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
        return lines[-1]

    product = run(None, True)
    for rows in (1, 2, 3, 5, 8):
        assert run({"PBR_SHADE_ROWS_BIG": str(rows)}, False) == product, f"rows {rows}: another image"
    assert run({"PBR_SHADE_ROWS_BIG": "4", "PBR_SHADE_BIGFRAC": "0.5", "PBR_SHADE_ROWS_SMALL": "3"}, False) == product
