"""pbr_shade_desc's own rules, through the raw library calls: which combinations of its fields pbr_deferred_shade and
pbr_deferred_shade_f32 refuse (PBR_ERR_INVALID under the name of the function that was called), and that no rectangle list means
the whole tile, bit for bit, for the sampled, folded and tabled forms.
Shapes (those of test_gpu_shade_lut_fold.py): the refusals on the 256 x 64 frame; the default rectangle on the 1536 x 64 frame
(staged lists, so the tabled form runs its own kernel), 256 lights, on a prefilled target."""
import ctypes as C

import numpy as np
import pytest
import torch

import common
from direct12pbrrenderer_amd import scene, synth
from direct12pbrrenderer_amd.structs import GBuffer, ShadeDesc, Tile

pytestmark = pytest.mark.gpu

ES, EM, LR = common.ENV_SIZE, common.ENV_MIPS, common.LUT_RES
FRAME = (0, 0, 1536, 64, 1536, 64)             # x0, y0, w, h, full_w, full_h
SMALL = (0, 0, 256, 64, 256, 64)
N_LIGHTS = 256
INVALID = -1


@pytest.fixture(scope="module")
def world(ctx, ibl):
    """LUT, folded table and padded env chain; per shape the scene, its culled lights and its shade tables with both halves built"""
    sky, env, lut, sh = ibl
    w = dict(lut=ctx.brdf_lut(LR), scene={})
    w["fold"] = ctx.lut_fold_x(w["lut"], LR)
    w["denv"] = ctx.env_pad(ctx.upload(np.ascontiguousarray(env, dtype=np.float16).view(np.uint16)).view(torch.float16), ES, EM)
    for shape in (FRAME, SMALL):
        x0, y0, tw, th, fw, fh = shape
        g = scene.make_global(scene.Camera.reference_default(fw, fh), fw, fh, sh_pack=sh)
        gb = {k: ctx.upload(v) for k, v in synth.gbuffer_tile(x0, y0, tw, th, fw, fh, rough_min=0, coverage_mask=True).items()}
        dl = ctx.upload(common.shade_scene(8, 8, N_LIGHTS, sh, full=(fw, fh))[2])
        cl = ctx.alloc_clusters()
        buf, tables = ctx.alloc_shade_tables(tw, th)
        ctx.shade_geometry_tables(Tile(*shape), tables)
        ctx.clustered_tables(g, dl, N_LIGHTS, cl, tables)
        w["scene"][shape] = (g, Tile(*shape), GBuffer(*[gb[k].data_ptr() for k in ("A", "B", "C", "depth", "stencil")], tw), gb, dl, cl, buf, tables)
    ctx.sync()
    return w


def desc(w, shape, hdr, **fields):
    """the descriptor of the shape's scene with neither LUT form, no rectangles and no tables; fields: what the case sets"""
    g, tile, gbs, gb, dl, cl, buf, tables = w["scene"][shape]
    d = ShadeDesc(g=C.addressof(g), tile=C.addressof(tile), gb=C.addressof(gbs), env_padded=w["denv"].data_ptr(), clusters=cl.data_ptr(),
                  lights=dl.data_ptr(), hdr=hdr.data_ptr() if hdr is not None else None, lut_res=LR, env_size=ES, env_mips=EM,
                  num_lights=N_LIGHTS, hdr_pitch=shape[2])
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def rect_list(rects):
    return ((C.c_uint32 * 4) * len(rects))(*[(C.c_uint32 * 4)(*r) for r in rects])


def test_refusals(ctx, world):
    x0, y0, tw, th, fw, fh = SMALL
    lib, tables = ctx.lib, world["scene"][SMALL][7]
    hdr = ctx.zeros((th, tw, 4), torch.float16)
    f32 = ctx.zeros((th, tw, 4), torch.float32)
    lut, fold = world["lut"].data_ptr(), world["fold"].data_ptr()
    one = rect_list([(0, 0, tw, th)])
    six = rect_list([(0, 0, tw, 8)] * 6)
    p_one, p_six, p_tables = C.addressof(one), C.addressof(six), C.addressof(tables)

    def half(**fields):
        d = desc(world, SMALL, hdr, **fields)
        return "pbr_deferred_shade", lib.pbr_deferred_shade(ctx.h, C.byref(d))

    def probe(**fields):
        d = desc(world, SMALL, fields.pop("hdr", None), **fields)
        return "pbr_deferred_shade_f32", lib.pbr_deferred_shade_f32(ctx.h, C.byref(d), f32.data_ptr())

    # what the refused cases are one field away from is accepted
    for call, fields in ((half, dict(lut=lut)), (half, dict(lut_fold=fold)), (half, dict(lut_fold=fold, tables=p_tables)),
                         (half, dict(lut=lut, rects=p_one, n_rects=1)), (probe, dict(lut=lut))):
        who, status = call(**fields)
        assert status == 0, f"{who} {sorted(fields)}: {lib.pbr_last_error(ctx.h)}"
    assert fold % 8 == 0
    refused = {
        "both LUT fields": (half, dict(lut=lut, lut_fold=fold)),
        "neither LUT field": (half, dict()),
        "tables with lut": (half, dict(lut=lut, tables=p_tables)),
        "no rectangle list, n_rects 1": (half, dict(lut=lut, n_rects=1)),
        "six rectangles": (half, dict(lut=lut, rects=p_six, n_rects=6)),
        "probe with lut_fold": (probe, dict(lut_fold=fold)),
        "probe with tables": (probe, dict(lut=lut, tables=p_tables)),
        "probe with rects": (probe, dict(lut=lut, rects=p_one, n_rects=1)),
        "probe with hdr": (probe, dict(lut=lut, hdr=hdr)),
        "lut_fold 4-byte aligned only": (half, dict(lut_fold=fold + 4)),
    }
    for name, (call, fields) in refused.items():
        who, status = call(**fields)
        assert status == INVALID, f"{name}: status {status}"
        assert lib.pbr_last_error(ctx.h).decode().startswith(who + ": "), f"{name}: {lib.pbr_last_error(ctx.h)}"
    ctx.sync()


@pytest.mark.parametrize("form", ["sampled", "folded", "tabled"])
def test_no_rectangle_list_is_the_whole_tile(ctx, world, form):
    x0, y0, tw, th, fw, fh = FRAME
    fields = dict(lut=world["lut"].data_ptr()) if form == "sampled" else dict(lut_fold=world["fold"].data_ptr())
    if form == "tabled":
        fields["tables"] = C.addressof(world["scene"][FRAME][7])
    whole = rect_list([(0, 0, tw, th)])
    bits = []
    for rects in (dict(), dict(rects=C.addressof(whole), n_rects=1)):
        hdr = torch.full((th, tw, 4), 3.0, dtype=torch.float16, device=ctx.torch_device)
        d = desc(world, FRAME, hdr, **fields, **rects)
        assert ctx.lib.pbr_deferred_shade(ctx.h, C.byref(d)) == 0, ctx.lib.pbr_last_error(ctx.h)
        bits.append(hdr.view(torch.int16).cpu().numpy())
    assert not np.all(bits[0] == np.float16(3.0).view(np.int16)), "nothing was shaded"
    assert np.array_equal(bits[0], bits[1]), f"{form}: rects = NULL, n_rects = 0 differs from the whole tile as one rectangle"
