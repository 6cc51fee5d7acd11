"""pbr_bloom_desc and pbr_bloom_prefilter_desc without a GPU: the ctypes mirrors BloomDesc and BloomPrefilterDesc have the header's
layout (and no padding), and the two entry points that take them refuse a null context."""
import ctypes as C
import os
import subprocess

import pytest

from test_multiview_cpu import ROOT, _host_compiler


@pytest.mark.parametrize("mirror, c_name, n_fields", [("BloomDesc", "pbr_bloom_desc", 15), ("BloomPrefilterDesc", "pbr_bloom_prefilter_desc", 13)])
def test_desc_layout_matches_the_header(tmp_path, mirror, c_name, n_fields):
    from direct12pbrrenderer_amd import structs
    desc = getattr(structs, mirror)
    fields = [f for f, _ in desc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pbr_hip.h"\nint main(void) {\n'
                   f'    printf("%zu\\n", sizeof({c_name}));\n'
                   + "".join(f'    printf("%zu\\n", offsetof({c_name}, {f}));\n' for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([_host_compiler(), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(desc)
    assert out[1:] == [getattr(desc, f).offset for f in fields]
    assert len(fields) == n_fields and out[0] == sum(C.sizeof(t) for _, t in desc._fields_), "a field is missing from the mirror, or the struct has padding"


def test_descriptor_entry_points_refuse_a_null_context():
    from direct12pbrrenderer_amd import _lib
    from direct12pbrrenderer_amd.structs import BloomDesc, BloomPrefilterDesc
    lib = _lib.load()
    assert lib.pbr_bloom(None, C.byref(BloomDesc())) == -1
    assert lib.pbr_bloom_prefilter(None, C.byref(BloomPrefilterDesc())) == -1
