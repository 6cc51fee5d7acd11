"""The multi-view sky entry points without a GPU: the symbols resolve and the calls refuse a null context."""
SKY_CALLS = ("pbr_skybox_views", "pbr_skybox_bc6h_views")


def test_symbols_resolve_and_refuse_a_null_context():
    from direct12pbrrenderer_amd import _lib
    from direct12pbrrenderer_amd.structs import CubeBc6h, CubeF32, View
    lib = _lib.load()
    for name in SKY_CALLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    views = (View * 2)()
    assert lib.pbr_skybox_views(None, views, 2, 64, 64, CubeF32()) == -1
    assert lib.pbr_skybox_bc6h_views(None, views, 2, 64, 64, CubeBc6h()) == -1


def test_header_declares_the_sky_view_calls():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "pbr_hip.h")).read()
    for name in SKY_CALLS:
        assert f"pbr_status {name}(pbr_ctx* ctx, const pbr_view* views, uint32_t n, uint32_t w, uint32_t h," in text, name
