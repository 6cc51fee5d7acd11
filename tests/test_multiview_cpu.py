"""Multi-view entry points without a GPU: the symbols resolve, a null context is refused, and the ctypes mirror of pbr_view has the
header's layout."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEW_CALLS = ("pbr_clustered_views", "pbr_deferred_shade_views", "pbr_bloom_histogram_views", "pbr_lum_average_views", "pbr_tonemap_views")


def test_view_symbols_resolve_and_refuse_a_null_context():
    from direct12pbrrenderer_amd import _lib
    from direct12pbrrenderer_amd.structs import View
    lib = _lib.load()
    for name in VIEW_CALLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    views = (View * 2)()
    assert lib.pbr_clustered_views(None, views, 2) == -1
    assert lib.pbr_deferred_shade_views(None, views, 2, 64, 64, None, 32, None, 16, 5) == -1
    assert lib.pbr_bloom_histogram_views(None, views, 2, 64, 64, 1.0, 0.5, -10.0, 1.0 / 12.0) == -1
    assert lib.pbr_lum_average_views(None, views, 2, 64 * 64, -10.0, 12.0) == -1
    assert lib.pbr_tonemap_views(None, views, 2, 64, 64) == -1


def _host_compiler():
    for cc in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang"):
        path = shutil.which(cc)
        if path:
            return path
    pytest.fail("no C compiler on this machine")


def test_view_struct_layout_matches_the_header(tmp_path):
    from direct12pbrrenderer_amd.structs import MAX_VIEWS, View
    fields = [f for f, _ in View._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pbr_hip.h"\nint main(void) {\n'
                   '    printf("%zu %d\\n", sizeof(pbr_view), PBR_MAX_VIEWS);\n'
                   + "".join(f'    printf("%zu\\n", offsetof(pbr_view, {f}));\n' for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([_host_compiler(), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert int(out[0]) == C.sizeof(View)
    assert int(out[1]) == MAX_VIEWS
    assert [int(v) for v in out[2:]] == [getattr(View, f).offset for f in fields]
