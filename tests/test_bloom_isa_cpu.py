"""Every kernel instantiation of bloom.hip stays within what profiles/bloom_isa_resources.md recorded for it ("new" rows): the same
LDS and occupancy, no scratch, no more registers, and no more v_*, ds_*, global_*, s_waitcnt or s_barrier instructions in the
cross-compiled gfx950 ISA (tools/isa_phase_count.py; scalar-ALU counts may move).  A change that is meant to leave the generated
code alone shows here when it does not; one that means to change it records a new table.  Instruction classes are counted, no
particular instruction is looked for.  No GPU; needs hipcc."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def load_tool():
    spec = importlib.util.spec_from_file_location("isa_phase_count", os.path.join(ROOT, "tools", "isa_phase_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tables():
    tool = load_tool()
    now = {name: row for name, (row, _) in tool.kernel_table(tool.compile_isa((), tool.BLOOM_SRC, tool.BLOOM_FLAGS)).items()}
    recorded = tool.parse_bloom_rows(open(os.path.join(ROOT, "profiles", "bloom_isa_resources.md")).read(), "new")
    return tool, now, recorded


def test_every_recorded_kernel_still_exists(tables):
    _, now, recorded = tables
    assert len(recorded) == 31, "profiles/bloom_isa_resources.md: the table lists 31 kernel instantiations"
    assert sorted(set(recorded) - set(now)) == []


def test_the_4k_frame_kernels_are_in_the_table(tables):
    _, _, recorded = tables
    frame = ["k_bloom_prefilter_2xIN3pbr7NoViewsE", "k_blur_hvILi1ELb0ELi0ELi32ELi512EN3pbr7NoViewsE", "k_blur_hvILi1ELb0ELi0ELi16ELi512EN3pbr7NoViewsE",
             "k_blur_hvILi2ELb1ELi0ELi16ELi512EN3pbr7NoViewsE", "k_blur_up_polyILb1ELi0ELi32EN3pbr7NoViewsE", "k_blur_up_polyILb0ELi2ELi32EN3pbr7NoViewsE"]
    for k in frame:
        assert any(k in name for name in recorded), k


def test_no_kernel_exceeds_its_recorded_row(tables):
    tool, now, recorded = tables
    over = {}
    for name, ref in recorded.items():
        if name in now:
            print(name, now[name])
            bad = tool.exceeds(now[name], ref)
            if bad:
                over[name] = {c: (now[name][c], ref[c]) for c in bad}
    assert over == {}, f"(now, recorded) per column: {over}"
