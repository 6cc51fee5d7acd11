"""pbr_gbuffer_raster with maps against the float64 truth of its sampler (tests/sampler_truth.py) on the inputs of
tests/sampler_cases.py: non-constant chains of every stored format, square, non-square, odd-sized, partial and BC1-resident, sampled
through uv fields that cross the wrap in both signs at every level pair and beyond both clamps of lambda.  Every covered pixel's A
(albedo), B (normal map) and C (roughness, metallic, AO) bytes must be admissible; nothing is set aside but the octahedral fold's sign
decisions on B.  tests/test_sampler_truth_cpu.py holds the restatement to the same truth on the same inputs and shows that the check
rejects each of a list of defects."""
import numpy as np
import pytest

import sampler_cases as C
import sampler_truth as S
from direct12pbrrenderer_amd import scene
from direct12pbrrenderer_amd.structs import TEX_BC1_BLOCKS
from test_gpu_raster_tex import gpu_raster_tex
from test_gpu_raster_truth import covered


def upload(ctx, mat):
    """(what keeps the device memory alive, the descriptors) of a material's table, decoded or BC1-resident"""
    keep = [ctx.upload_texture(t.blocks, t.width, t.height, t.mips, t.format | TEX_BC1_BLOCKS) if t.blocks is not None else
            ctx.upload_texture(scene.pack_chain(t.levels), t.width, t.height, t.mips, t.format) for t in mat.table]
    return keep, [k[1] for k in keep]


def planes(ctx, case, mat, fld, descs):
    v, i, d, maps = C.draw(case, mat, fld)
    got = gpu_raster_tex(ctx, case.g, case.tile, v, i, d, maps, [], descs=descs)
    covered(case, got)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("case", C.CASES, ids=repr)
@pytest.mark.parametrize("mat", C.MATERIALS, ids=repr)
def test_sampled_bytes_admissible(ctx, case, mat):
    """one launch per field; the worst share of each plane's allowance and of A's transcendental band are printed (above 1.0 of the
    latter the 1 ULP figure of gbuffer_encode.hpp's comment would be wrong: that is then a failure of A)"""
    keep, descs = upload(ctx, mat)
    worst = C.Worst()
    for fld in C.fields(mat, case):
        st = C.check(case, mat, fld, planes(ctx, case, mat, fld, descs))
        worst.add(st)
        bad, ok = C.verdict(st)
        print(C.describe(f"  t {fld[0]:.4g} base {fld[1]}", st))
        assert bad == 0 and ok, (fld, st)
    del keep
    print(f"{case} {mat}: GPU, {len(case.geometry[2])} pixels x {len(C.fields(mat, case))} fields, worst: {worst}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", C.FLAT, ids=repr)
@pytest.mark.parametrize("mat", [m for m in C.MATERIALS if m.format != S.B8G8R8A8_SRGB], ids=repr)
def test_exact_field_reads_texel_bytes(ctx, case, mat):
    """every pixel centre on a texel centre: C's three bytes are the texel's red byte, on decoded and on BC1-resident chains"""
    keep, descs = upload(ctx, mat)
    got = planes(ctx, case, mat, C.EXACT, descs)
    del keep
    _, _, ys, xs, _ = case.geometry
    want = C.exact_texel_bytes(case, mat.tex("surface"))
    for shift in (0, 8, 16):
        assert np.array_equal((got["C"][ys, xs].astype(np.int64) >> shift) & 255, want), shift
