"""pbr_depth_raster without a GPU: the ctypes mirror DepthRasterDesc has the header's layout (and no padding), the entry point refuses
a null context, and the depth layout's scratch lies at least the 80-byte resolve record per triangle below the G-buffer raster's."""
import ctypes as C
import os
import subprocess

import pytest

from test_multiview_cpu import ROOT, _host_compiler


def test_depth_raster_desc_layout_matches_the_header(tmp_path):
    from direct12pbrrenderer_amd.structs import DepthRasterDesc
    fields = [f for f, _ in DepthRasterDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pbr_hip.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(pbr_depth_raster_desc));\n'
                   + "".join(f'    printf("%zu\\n", offsetof(pbr_depth_raster_desc, {f}));\n' for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([_host_compiler(), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(DepthRasterDesc)
    assert out[1:] == [getattr(DepthRasterDesc, f).offset for f in fields]
    assert len(fields) == 16 and out[0] == 104 == sum(C.sizeof(t) for _, t in DepthRasterDesc._fields_), \
        "a field is missing from the mirror, or the struct has padding"
    # 8-byte fields first
    sizes = [C.sizeof(t) for _, t in DepthRasterDesc._fields_]
    assert sizes == sorted(sizes, reverse=True)


def test_entry_point_refuses_a_null_context():
    from direct12pbrrenderer_amd import _lib
    from direct12pbrrenderer_amd.structs import DepthRasterDesc
    lib = _lib.load()
    assert lib.pbr_depth_raster(None, C.byref(DepthRasterDesc())) == -1


@pytest.mark.parametrize("w,h,n", [(16, 16, 1), (257, 131, 3000), (2048, 2048, 48576)])
def test_scratch_drops_the_resolve_records(w, h, n):
    from direct12pbrrenderer_amd import _lib
    lib = _lib.load()
    depth_min, depth_rec = lib.pbr_depth_raster_min_scratch_bytes(w, h, n), lib.pbr_depth_raster_scratch_bytes(w, h, n)
    gbuffer_min = lib.pbr_gbuffer_raster_min_scratch_bytes(w, h, n)
    assert 0 < depth_min <= gbuffer_min - 80 * n, (depth_min, gbuffer_min)
    assert depth_rec >= depth_min
