"""pbr_gbuffer_raster's coverage, depth, winner and stencil on the GPU against the float64 truth of tests/raster_cover_truth.py: one
gpu_raster call per case through the assertion function tests/test_raster_cover_truth_cpu.py holds the restatement to (coverage and
clear values by the decided verdicts, depth inside its band, winner byte and stencil where decided, both caps); the special
triangles' minimums; the floor through the near plane and the guard band as one surface, in eight draws, in one, with the minimum
scratch, and as a tile with its own origin and pitch."""
import pytest

import raster_cover_truth as T
from direct12pbrrenderer_amd.structs import Tile
from test_gpu_raster import gpu_raster, same


@pytest.mark.gpu
@pytest.mark.parametrize("name", T.CASE_NAMES)
def test_kernel_inside_the_truth(ctx, name):
    case = T.case(name)
    got = gpu_raster(ctx, case.g, case.tile, *case.scene(), pitch=case.pitch)
    res = T.check(case.truth, got, what=name)
    print(T.report(name, res))
    # the pixels each special kind has to win (check() has held the kernel's winner byte to the truth's on every one of them)
    for kind, draws in case.kinds.items():
        won = case.truth.won_pixels(draws[:1])
        assert won >= (T.SPECIAL_MIN if name.startswith("regimes") else 1), (kind, won)


@pytest.mark.gpu
@pytest.mark.parametrize("name", T.FLOOR_NAMES)
def test_floor_is_one_surface(ctx, name):
    """the floors of raster_cover_truth.floor() (the low and the fine ones have the near line, guard-cut triangles and shared edges of
    clipped polygons inside the frame): no hole and no double hit on any pixel decided inside the floor's visible part, a depth within
    the band of the planes of the triangles that may hold the pixel, clear values outside;
    the whole floor in one draw and the minimum scratch (the bin walk without lists) give the same bits; so does a 101 x 53 tile at
    (37, 19) with pitch w + 5"""
    case = T.case(name)
    v, i, d = case.scene()
    got = gpu_raster(ctx, case.g, case.tile, v, i, d)
    res = T.check(case.truth, got, winners=False, what=name)
    print(T.report(name, res))
    assert res["decided"] > 5000
    same(got, gpu_raster(ctx, case.g, case.tile, *case.scene(one_draw=True)))
    same(got, gpu_raster(ctx, case.g, case.tile, v, i, d, minimum=True))
    tile = Tile(*T.FLOOR_TILE, *case.full)
    part = gpu_raster(ctx, case.g, tile, v, i, d, pitch=tile.w + 5)
    print(T.report(f"{name} tile", T.check(case.truth, part, tile=tile, winners=False, what=f"{name} tile")))
    same(part, {k: a[tile.y0:tile.y0 + tile.h, tile.x0:tile.x0 + tile.w] for k, a in got.items()})
