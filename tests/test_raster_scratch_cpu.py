"""The six scratch-size exports of the rasterizer return what they have returned since they were added: 18 recorded values, literals
below.  PbrContext's six helpers (raster_ / depth_raster_ / textured_raster_scratch_bytes and their alloc_ forms) return the same
numbers and allocate tensors of that size plus `extra`; the allocation needs a device."""
import pytest
import torch

SHAPES = [(16, 16, 1), (257, 131, 3000), (2048, 2048, 48576)]
# export -> its value at each of SHAPES
RECORDED = {
    "pbr_gbuffer_raster_min_scratch_bytes": [263936, 841216, 9785856],
    "pbr_gbuffer_raster_scratch_bytes": [264192, 939776, 11602432],
    "pbr_gbuffer_raster_textured_min_scratch_bytes": [264192, 1033216, 12894720],
    "pbr_gbuffer_raster_textured_scratch_bytes": [264448, 1131776, 14711296],
    "pbr_depth_raster_min_scratch_bytes": [263680, 601088, 5899776],
    "pbr_depth_raster_scratch_bytes": [263936, 699648, 7716352],
}
# PbrContext helper (and its alloc_ form) -> (the minimum's export, the recommended size's export)
HELPERS = {
    "raster_scratch_bytes": ("pbr_gbuffer_raster_min_scratch_bytes", "pbr_gbuffer_raster_scratch_bytes"),
    "textured_raster_scratch_bytes": ("pbr_gbuffer_raster_textured_min_scratch_bytes", "pbr_gbuffer_raster_textured_scratch_bytes"),
    "depth_raster_scratch_bytes": ("pbr_depth_raster_min_scratch_bytes", "pbr_depth_raster_scratch_bytes"),
}


@pytest.mark.parametrize("export", sorted(RECORDED))
def test_exports_return_the_recorded_sizes(export):
    from direct12pbrrenderer_amd import _lib
    fn = getattr(_lib.load(), export)
    assert [int(fn(*s)) for s in SHAPES] == RECORDED[export]


def _sizes():
    """a PbrContext without a device: the size helpers use its library alone"""
    from direct12pbrrenderer_amd import _lib
    from direct12pbrrenderer_amd.api import PbrContext
    c = PbrContext.__new__(PbrContext)
    c.lib = _lib.load()
    return c


@pytest.mark.parametrize("helper", sorted(HELPERS))
def test_helpers_return_the_recorded_sizes(helper):
    fn = getattr(_sizes(), helper)
    least, recommended = HELPERS[helper]
    for k, s in enumerate(SHAPES):
        assert fn(*s, minimum=True) == RECORDED[least][k] and fn(*s) == fn(*s, False) == RECORDED[recommended][k]


@pytest.mark.gpu
@pytest.mark.parametrize("helper", sorted(HELPERS))
def test_alloc_helpers_allocate_that_size_plus_extra(ctx, helper):
    alloc = getattr(ctx, "alloc_" + helper[:-len("_bytes")])
    least, recommended = HELPERS[helper]
    for minimum, export in ((True, least), (False, recommended)):
        for extra in (0, 52):
            t = alloc(16, 16, 1, minimum=minimum, extra=extra)
            assert t.dtype == torch.uint8 and t.is_cuda and tuple(t.shape) == (RECORDED[export][0] + extra,)
    assert alloc(16, 16, 1).numel() == RECORDED[recommended][0]
