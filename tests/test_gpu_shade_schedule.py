"""The pieces the shade kernels share — a block's span of its rectangle, the column and row terms, the pick of the kernel — at the shapes
where they can go wrong, every form of the shade against the others.
Shapes: a 600 x 37 tile at (1000, 700) of a 4K frame (three column blocks, the last one partial; long blocks of two rows, one-row tail
blocks; staged lists), whole and as five rectangles (one a pixel wide, one 257 wide, one a row high); a 328 x 37 frame (global lists);
two views of 3072 x 64 (staged) and of 328 x 37 (global) with different cameras and light counts.  0, 3 and 300 lights: both strides
of the LDS light table.
Asserted, on prefilled targets compared as bits:
  * the forms that run the same shade_pixel instantiation — sampled whole / rectangles / views, folded whole / rectangles / tabled —
    write the same bits to the pixels they own; the folded and tabled forms write the sampled whole-tile shade's bits;
  * every covered pixel a form owns is written (alpha 1); the fp32 probe, an instantiation of its own, rounded to half (nearest even, what
    the fp16 store does) is within ONE half step of the sampled target: the two evaluate one fp32 expression in two instruction orders,
    whose difference (a few fp32 ulps, 2^-13 of a half step each) can only move a value across a rounding boundary — it does at one
    pixel of 22 200 with 300 lights — while a wrong column or row term moves it by many steps;
  * every pixel outside the rectangles or with stencil 0 keeps the prefill;
  * the launch log names the kernel the case is meant to take."""
import numpy as np
import pytest
import torch

import common
from direct12pbrrenderer_amd import scene, synth
from direct12pbrrenderer_amd.structs import GBuffer, Tile, View

pytestmark = pytest.mark.gpu

ES, EM, LR = common.ENV_SIZE, common.ENV_MIPS, 32
TILE_4K = (1000, 700, 600, 37, 3840, 2160)     # x0, y0, w, h, full_w, full_h
SMALL = (0, 0, 328, 37, 328, 37)
WIDE = (0, 0, 3072, 64, 3072, 64)
RECTS = [(5, 3, 1, 30), (10, 0, 257, 20), (300, 5, 200, 1), (300, 10, 300, 27), (10, 22, 280, 15)]   # disjoint, tile-local x, y, w, h
LIGHTS = (0, 3, 300)
PREFILL = np.float16(3.0).view(np.int16)


def camera(fw, fh, yaw=0.0):
    cam = scene.Camera.reference_default(fw, fh)
    if yaw:
        cam.rotate(0.0, yaw, 0.0)
    return cam


def make_world(ctx, ibl):
    sky, env, lut, sh = ibl
    w = dict(sh=sh, scene={}, cull={}, shaded={})
    w["denv"] = ctx.env_pad(ctx.upload(np.ascontiguousarray(env, dtype=np.float16).view(np.uint16)).view(torch.float16), ES, EM)
    w["lut"] = ctx.brdf_lut(LR)
    w["fold"] = ctx.lut_fold_x(w["lut"], LR)
    for shape, yaw in ((TILE_4K, 0.0), (SMALL, 0.0), (WIDE, 0.0), (SMALL, 0.3), (WIDE, 0.3)):
        x0, y0, tw, th, fw, fh = shape
        cam = camera(fw, fh, yaw)
        gb = synth.gbuffer_tile(x0, y0, tw, th, fw, fh, rough_min=0, coverage_mask=True)
        w["scene"][shape, yaw] = (cam, scene.make_global(cam, fw, fh, sh_pack=sh), {k: ctx.upload(v) for k, v in gb.items()}, gb["stencil"] > 0)
    ctx.sync()
    return w


@pytest.fixture(scope="module")
def world(ctx, ibl):
    return make_world(ctx, ibl)


def culled(ctx, w, shape, n, yaw=0.0):
    """(device lights or None, cluster table, shade tables) of n lights culled for the scene's camera, both halves of the tables built"""
    key = (shape, n, yaw)
    if key not in w["cull"]:
        cam, g = w["scene"][shape, yaw][:2]
        dl = ctx.upload(synth.lights_in_view_box(n, cam)) if n else None
        cl = ctx.alloc_clusters()
        buf, tables = ctx.alloc_shade_tables(shape[2], shape[3])
        ctx.shade_geometry_tables(Tile(*shape), tables)
        ctx.clustered_tables(g, dl, n, cl, tables)
        w["cull"][key] = (dl, cl, buf, tables)
    return w["cull"][key]


def shade(ctx, w, shape, n, form, rects=None, yaw=0.0):
    """(HDR target as int16 — the probe's as float32 —, labels of the launches) of one single-view form, made once per case"""
    key = (shape, n, form, rects is not None, yaw)
    if key not in w["shaded"]:
        tw, th = shape[2:4]
        cam, g, gbd, on = w["scene"][shape, yaw]
        dl, cl, buf, tables = culled(ctx, w, shape, n, yaw)
        probe = form == "f32"
        out = torch.full((th, tw, 4), 3.0, dtype=torch.float32 if probe else torch.float16, device=ctx.torch_device)
        head = (g, Tile(*shape), gbd, tw)
        tail = (LR, w["denv"], ES, EM, cl, dl, n, out, tw)
        call = {"sampled": lambda: ctx.deferred_shade_rects(*head, w["lut"], *tail, rects) if rects else ctx.deferred_shade(*head, w["lut"], *tail),
                "folded": lambda: ctx.deferred_shade_folded(*head, w["fold"], *tail, rects),
                "tabled": lambda: ctx.deferred_shade_tabled(*head, w["fold"], *tail, tables, rects),
                "f32": lambda: ctx.deferred_shade_f32(*head, w["lut"], *tail)}[form]
        labels = ctx.launches_of(call)
        w["shaded"][key] = (out.cpu().numpy() if probe else out.view(torch.int16).cpu().numpy(), labels)
    return w["shaded"][key]


def owned(shape, on, rects):
    inside = np.zeros(on.shape, dtype=bool)
    for x, y, rw, rh in rects or [(0, 0, shape[2], shape[3])]:
        inside[y:y + rh, x:x + rw] = True
    return inside & on


def same_bits(a, b, where, what):
    bad = np.argwhere((a != b).any(axis=2) & where)
    assert bad.size == 0, f"{what}: {len(bad)} pixels differ, first at (y, x) = {tuple(bad[0])}"


@pytest.mark.parametrize("n", LIGHTS)
@pytest.mark.parametrize("shape", [TILE_4K, SMALL], ids=["tile_of_4k", "small_frame"])
def test_whole_tile_forms(ctx, world, shape, n):
    on = world["scene"][shape, 0.0][3]
    ref, labels = shade(ctx, world, shape, n, "sampled")
    assert labels == ["k_deferred_shade"]
    assert on.sum() > 0.3 * on.size and not on.all() and not np.all(ref[on][:, :3] == PREFILL)
    assert np.all(ref[~on] == PREFILL), "a pixel with stencil 0 was written"
    assert np.all(ref[on][:, 3] == np.float16(1.0).view(np.int16)), "a covered pixel was not written"
    staged = shape == TILE_4K
    for form, label in (("folded", "k_deferred_shade"), ("tabled", "k_deferred_shade_tabled" if staged else "k_deferred_shade")):
        got, labels = shade(ctx, world, shape, n, form)
        assert labels == [label], form
        same_bits(got, ref, np.ones_like(on), f"{form}, {n} lights")
    probe, labels = shade(ctx, world, shape, n, "f32")
    assert labels == ["k_deferred_shade"]
    assert np.all(probe[~on] == 3.0) and np.isfinite(probe[on]).all() and np.all(probe[on][:, 3] == 1.0)
    with np.errstate(over="ignore"):
        steps = common.half_ulp_diff(probe[on].astype(np.float16), ref.view(np.float16)[on])
    print(f"fp32 probe rounded to half against the sampled target, {n} lights: {int((steps > 0).sum())} values differ, at most {int(steps.max())} half steps")
    assert steps.max() <= 1


@pytest.mark.parametrize("n", LIGHTS)
def test_rectangles(ctx, world, n):
    on = world["scene"][TILE_4K, 0.0][3]
    mine = owned(TILE_4K, on, RECTS)
    assert mine.sum() > 2000 and (on & ~mine).sum() > 2000
    whole = shade(ctx, world, TILE_4K, n, "sampled")[0]
    for form, label in (("sampled", "k_deferred_shade"), ("folded", "k_deferred_shade"), ("tabled", "k_deferred_shade_tabled")):
        got, labels = shade(ctx, world, TILE_4K, n, form, RECTS)
        assert labels == [label], form
        same_bits(got, whole, mine, f"{form} on rectangles, {n} lights")
        assert np.all(got[~mine] == PREFILL), f"{form}: a pixel outside the rectangles or with stencil 0 was written"


VIEW_YAWS = (0.0, 0.3)
VIEW_COUNTS = [(0, 3), (3, 300)]


def shade_views(ctx, w, shape, counts):
    """(one HDR target as int16 per view, labels of the launches) of one multi-view launch: view k has VIEW_YAWS[k]'s camera and counts[k] lights"""
    tw, th = shape[2:4]
    hdrs, views = [], (View * len(counts))()
    for k, (n, yaw) in enumerate(zip(counts, VIEW_YAWS)):
        gbd = w["scene"][shape, yaw][2]
        dl, cl, buf, tables = culled(ctx, w, shape, n, yaw)
        hdrs.append(torch.full((th, tw, 4), 3.0, dtype=torch.float16, device=ctx.torch_device))
        views[k].g = w["scene"][shape, yaw][1]
        views[k].gb = GBuffer(*[gbd[p].data_ptr() for p in ("A", "B", "C", "depth", "stencil")], tw)
        views[k].lights, views[k].num_lights, views[k].clusters = (dl.data_ptr() if n else None), n, cl.data_ptr()
        views[k].hdr, views[k].hdr_pitch = hdrs[k].data_ptr(), tw
    labels = ctx.launches_of(lambda: ctx.deferred_shade_views(views, len(counts), tw, th, w["lut"], LR, w["denv"], ES, EM))
    return [h.view(torch.int16).cpu().numpy() for h in hdrs], labels


@pytest.mark.parametrize("counts", VIEW_COUNTS, ids=["stride_257", "stride_1025"])
@pytest.mark.parametrize("shape", [WIDE, SMALL], ids=["staged", "global_lists"])
def test_views(ctx, world, shape, counts):
    """two views, the second with a yawed camera and its own lights: each is its single-view sampled shade, whatever the batch's light stride"""
    got, labels = shade_views(ctx, world, shape, counts)
    assert labels == ["k_deferred_shade<views>"]
    for k, (n, yaw) in enumerate(zip(counts, VIEW_YAWS)):
        on = world["scene"][shape, yaw][3]
        ref = shade(ctx, world, shape, n, "sampled", yaw=yaw)[0]
        assert not np.all(got[k][on][:, :3] == PREFILL)
        same_bits(got[k], ref, np.ones_like(on), f"view {k}, {n} lights")
