"""Every refusal of pbr_gbuffer_raster and pbr_depth_raster, pinned to the exact text pbr_last_error gives for it: the two entry points
share their checks, and each refuses under its own name.  The expected messages are literals (include/pbr_hip.h documents the refusals),
not read from the library.  Two descriptors carry two faults each and fix which refusal comes first: a null `vertices` with a bad tile
(the null-pointer check precedes the tile check), and a bad texture with a null `g` (the texture table is checked before the pointers).
A refused call enqueues nothing: the targets hold a sentinel throughout.  The stencil plane is bytes and has no alignment to refuse: a
descriptor with an odd stencil address is accepted."""
import ctypes as C

import numpy as np
import pytest
import torch

from direct12pbrrenderer_amd.structs import (DRAW_MAPS_DTYPE, NO_MAP, TEX_R8G8B8A8_UNORM, DepthRasterDesc, RasterDesc, Texture2D, Tile)
from test_gpu_raster import random_scene

pytestmark = pytest.mark.gpu

W, H, PITCH = 40, 24, 43
SENTINEL = 0x7FC5A5A5       # a quiet NaN no kernel writes


class Setup:
    """one 40 x 24 tile and 32 random triangles on the device, with targets for both entry points"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.g, self.v, self.i, self.d = random_scene(W, H, 7, n=32)
        self.n = int((self.d["index_count"] // 3).sum())
        self.tile = Tile(0, 0, W, H, W, H)
        self.dv, self.di, self.dd = ctx.upload(self.v), ctx.upload(self.i), ctx.upload(self.d)
        self.stats = ctx.alloc_cull_stats()
        self.bounds = ctx.upload(np.zeros(len(self.d) * 6, np.float32))
        maps = np.zeros(len(self.d), DRAW_MAPS_DTYPE)
        for name in DRAW_MAPS_DTYPE.names:
            maps[name] = NO_MAP
        self.maps = ctx.upload(maps)
        self.texels = ctx.zeros((4 * 4 * 4 + 16,), torch.uint8)          # a 4 x 4 RGBA8 level, and room behind a misaligned start
        self.tiles = []                                                  # the bad tiles, kept alive
        # four 32-bit planes (A, B, C, depth) and the stencil bytes (one spare: the odd stencil address of the accepted call)
        self.planes = [ctx.empty((H, PITCH), torch.int32).fill_(SENTINEL) for _ in range(4)]
        self.stencil = ctx.empty((H * PITCH + 1,), torch.uint8).fill_(0xA5)
        self.depth_only = ctx.empty((H, PITCH), torch.int32).fill_(SENTINEL)

    def untouched(self):
        self.ctx.sync()
        return (all(bool((p == SENTINEL).all()) for p in self.planes + [self.depth_only]) and bool((self.stencil == 0xA5).all()))

    def bad_tile(self, *a):
        self.tiles.append(Tile(*a))
        return C.addressof(self.tiles[-1])

    def table(self, *textures):
        self.tiles.append((Texture2D * len(textures))(*textures))
        return C.addressof(self.tiles[-1])


@pytest.fixture(scope="module")
def s(ctx):
    return Setup(ctx)


def check(s, fn, cases):
    for what, (dsc, message) in cases.items():
        assert fn(s.ctx.h, None if dsc is None else C.byref(dsc)) == -1, what
        got = (s.ctx.lib.pbr_last_error(s.ctx.h) or b"").decode()
        print(f"{what} -> {got}")
        assert got == message, what
    assert s.untouched()


def shared_cases(who, desc, s, planes):
    """the refusals both entry points have: (descriptor, message) by name; planes: {field: device address} of the call's 32-bit targets"""
    dv, di, dd = s.dv.data_ptr(), s.di.data_ptr(), s.dd.data_ptr()
    null, empty, limits = f"{who}: null pointer", f"{who}: empty vertex / index / draw list", f"{who}: more draws or triangles than the limits"
    tile, unaligned = f"{who}: bad tile", f"{who}: unaligned buffer"
    cases = {f"null {f}": (desc(**{f: None}), null) for f in ["g", "tile", "vertices", "indices", "draws", "scratch"] + list(planes)}
    cases.update({f"{f} misaligned": (desc(**{f: a + 2}), unaligned) for f, a in planes.items()})
    cases.update({
        "null descriptor": (None, f"{who}: null descriptor"),
        "no vertices": (desc(n_vertices=0), empty), "no indices": (desc(n_indices=0), empty), "no draws": (desc(n_draws=0), empty),
        "no triangles": (desc(max_triangles=0), empty),
        "too many draws": (desc(n_draws=65536 + 1), limits), "too many triangles": (desc(max_triangles=(1 << 22) + 1), limits),
        "empty tile": (desc(tile=s.bad_tile(0, 0, 0, H, W, H)), tile), "tile outside its frame": (desc(tile=s.bad_tile(8, 0, W, H, W, H)), tile),
        "frame too large": (desc(tile=s.bad_tile(0, 0, W, H, 8192 + 1, H)), tile), "empty frame": (desc(tile=s.bad_tile(0, 0, W, H, 0, 0)), tile),
        "pitch < w": (desc(pitch=W - 1), f"{who}: pitch < tile width"),
        "vertices misaligned": (desc(vertices=dv + 2), unaligned), "indices misaligned": (desc(indices=di + 1), unaligned),
        "draws misaligned": (desc(draws=dd + 2), unaligned),
        "scratch misaligned": (desc(scratch=s.scratch.data_ptr() + 8, scratch_bytes=s.scratch.numel() - 8), unaligned),
        "bounds misaligned": (desc(bounds=s.bounds.data_ptr() + 2), f"{who}: bounds not 4-byte aligned"),
        "stats misaligned": (desc(bounds=s.bounds.data_ptr(), stats=s.stats.data_ptr() + 2), f"{who}: stats not 4-byte aligned"),
        "stats without bounds": (desc(stats=s.stats.data_ptr()), f"{who}: stats without bounds"),
        # two faults: the null-pointer check comes before the tile check
        "null vertices and a bad tile": (desc(vertices=None, tile=s.bad_tile(8, 0, W, H, W, H)), null),
    })
    return cases


def test_depth_raster_refusals(ctx, s):
    s.scratch = ctx.alloc_depth_raster_scratch(W, H, s.n)
    least = ctx.depth_raster_scratch_bytes(W, H, s.n, minimum=True)

    def desc(**over):
        f = dict(g=C.addressof(s.g), tile=C.addressof(s.tile), vertices=s.dv.data_ptr(), indices=s.di.data_ptr(), draws=s.dd.data_ptr(),
                 depth=s.depth_only.data_ptr(), scratch=s.scratch.data_ptr(), scratch_bytes=s.scratch.numel(), bounds=None, stats=None,
                 n_vertices=len(s.v), n_indices=len(s.i), n_draws=len(s.d), max_triangles=s.n, pitch=PITCH, reserved=0)
        f.update(over)
        return DepthRasterDesc(**f)

    who = "pbr_depth_raster"
    cases = shared_cases(who, desc, s, {"depth": s.depth_only.data_ptr()})
    cases.update({
        "scratch below the minimum": (desc(scratch_bytes=least - 1), f"{who}: scratch below pbr_depth_raster_min_scratch_bytes"),
        "reserved": (desc(reserved=1), f"{who}: reserved is not 0"),
    })
    assert len(cases) == 28 + 2          # the 28 descriptors of test_gpu_depth_raster.py, the null descriptor, the one with two faults
    check(s, ctx.lib.pbr_depth_raster, cases)
    assert ctx.lib.pbr_depth_raster(ctx.h, C.byref(desc(scratch_bytes=least))) == 0          # the minimum itself is accepted
    ctx.sync()
    assert not bool((s.depth_only[:, :W] == SENTINEL).any())
    s.depth_only.fill_(SENTINEL)


def test_gbuffer_raster_refusals(ctx, s):
    s.scratch = ctx.alloc_textured_raster_scratch(W, H, s.n)
    least = ctx.raster_scratch_bytes(W, H, s.n, minimum=True)
    least_textured = ctx.textured_raster_scratch_bytes(W, H, s.n, minimum=True)
    A, B, Cc, depth = (p.data_ptr() for p in s.planes)

    def desc(**over):
        f = dict(g=C.addressof(s.g), tile=C.addressof(s.tile), vertices=s.dv.data_ptr(), indices=s.di.data_ptr(), draws=s.dd.data_ptr(),
                 A=A, B=B, C=Cc, depth=depth, stencil=s.stencil.data_ptr(), scratch=s.scratch.data_ptr(), scratch_bytes=s.scratch.numel(),
                 n_vertices=len(s.v), n_indices=len(s.i), n_draws=len(s.d), max_triangles=s.n, pitch=PITCH)
        f.update(over)
        return RasterDesc(**f)

    def tex(texels=s.texels.data_ptr(), width=4, height=4, mips=1, fmt=TEX_R8G8B8A8_UNORM):
        return Texture2D(texels, width, height, mips, fmt)

    def textured(*textures, n=None, **over):
        return desc(**dict(dict(maps=s.maps.data_ptr(), textures=s.table(*textures) if textures else None,
                                n_textures=len(textures) if n is None else n), **over))

    who = "pbr_gbuffer_raster"
    table = f"{who}: more textures than PBR_RASTER_MAX_TEXTURES, or a null texture table"
    texels = f"{who}: texels null or not aligned to the texel size (BC1 blocks: 8 bytes)"
    cases = shared_cases(who, desc, s, {"A": A, "B": B, "C": Cc, "depth": depth})
    cases.update({
        "null stencil": (desc(stencil=None), f"{who}: null pointer"),
        "textures without maps": (desc(textures=s.table(tex()), n_textures=1), f"{who}: textures or n_textures without maps"),
        "n_textures without maps": (desc(n_textures=1), f"{who}: textures or n_textures without maps"),
        "maps misaligned": (textured(tex(), maps=s.maps.data_ptr() + 2), f"{who}: maps not 4-byte aligned"),
        "too many textures": (textured(tex(), n=64 + 1), table),
        "null table with n_textures": (textured(n=1), table),
        "null texels": (textured(tex(), tex(texels=None)), texels),
        "texels misaligned": (textured(tex(texels=s.texels.data_ptr() + 2)), texels),
        "unknown texture format": (textured(tex(fmt=29)), f"{who}: unknown texture format"),
        "texture of width 0": (textured(tex(width=0)), f"{who}: texture size zero or above PBR_TEX_MAX_SIZE"),
        "texture too large": (textured(tex(height=16384 + 1)), f"{who}: texture size zero or above PBR_TEX_MAX_SIZE"),
        "too many mip levels": (textured(tex(mips=4)), f"{who}: mip_levels 0 or above floor(log2(min(w, h))) + 1"),
        "no mip levels": (textured(tex(mips=0)), f"{who}: mip_levels 0 or above floor(log2(min(w, h))) + 1"),
        # two faults: the texture table is checked before the pointers
        "a bad texture and a null g": (textured(tex(fmt=29), g=None), f"{who}: unknown texture format"),
        "scratch below the minimum": (desc(scratch_bytes=least - 1), f"{who}: scratch below pbr_gbuffer_raster_min_scratch_bytes"),
        "scratch below the textured minimum": (textured(tex(), scratch_bytes=least_textured - 1),
                                               f"{who}: scratch below pbr_gbuffer_raster_textured_min_scratch_bytes"),
    })
    check(s, ctx.lib.pbr_gbuffer_raster, cases)
    # accepted: both minima themselves, and a stencil plane at an odd address (bytes: there is no alignment to refuse)
    assert least < least_textured
    assert ctx.lib.pbr_gbuffer_raster(ctx.h, C.byref(textured(tex(), scratch_bytes=least_textured))) == 0
    assert ctx.lib.pbr_gbuffer_raster(ctx.h, C.byref(desc(scratch_bytes=least, stencil=s.stencil.data_ptr() + 1))) == 0
    ctx.sync()
    assert not any(bool((p[:, :W] == SENTINEL).any()) for p in s.planes)
