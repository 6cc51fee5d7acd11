"""pbr_raster_desc without a GPU: the ctypes mirror RasterDesc has the header's layout (and no padding), the one entry point refuses
a null context, and the three entry points it replaced are gone from the library."""
import ctypes as C
import os
import subprocess

from test_multiview_cpu import ROOT, _host_compiler


def test_raster_desc_layout_matches_the_header(tmp_path):
    from direct12pbrrenderer_amd.structs import RasterDesc
    fields = [f for f, _ in RasterDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pbr_hip.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(pbr_raster_desc));\n'
                   + "".join(f'    printf("%zu\\n", offsetof(pbr_raster_desc, {f}));\n' for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([_host_compiler(), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(RasterDesc)
    assert out[1:] == [getattr(RasterDesc, f).offset for f in fields]
    assert len(fields) == 22 and out[0] == 152 == sum(C.sizeof(t) for _, t in RasterDesc._fields_), \
        "a field is missing from the mirror, or the struct has padding"


def test_one_entry_point_that_refuses_a_null_context():
    from direct12pbrrenderer_amd import _lib
    from direct12pbrrenderer_amd.structs import RasterDesc
    lib = _lib.load()
    assert lib.pbr_gbuffer_raster(None, C.byref(RasterDesc())) == -1
    for gone in ("textured", "culled", "textured_culled"):
        assert not hasattr(lib, "pbr_gbuffer_raster_" + gone), f"pbr_gbuffer_raster_{gone} is still exported"
