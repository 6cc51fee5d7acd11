"""pbr_shade_desc without a GPU: the ctypes mirror ShadeDesc has the header's layout (and no padding), and both entry points that take
the descriptor refuse a null context."""
import ctypes as C
import os
import subprocess

from test_multiview_cpu import ROOT, _host_compiler


def test_shade_desc_layout_matches_the_header(tmp_path):
    from direct12pbrrenderer_amd.structs import ShadeDesc
    fields = [f for f, _ in ShadeDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pbr_hip.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(pbr_shade_desc));\n'
                   + "".join(f'    printf("%zu\\n", offsetof(pbr_shade_desc, {f}));\n' for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([_host_compiler(), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(ShadeDesc)
    assert out[1:] == [getattr(ShadeDesc, f).offset for f in fields]
    assert len(fields) == 17 and out[0] == sum(C.sizeof(t) for _, t in ShadeDesc._fields_), "a field is missing from the mirror, or the struct has padding"


def test_descriptor_entry_points_refuse_a_null_context():
    from direct12pbrrenderer_amd import _lib
    from direct12pbrrenderer_amd.structs import ShadeDesc
    lib = _lib.load()
    d = ShadeDesc()
    assert lib.pbr_deferred_shade(None, C.byref(d)) == -1
    assert lib.pbr_deferred_shade_f32(None, C.byref(d), None) == -1
