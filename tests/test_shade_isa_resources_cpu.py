"""Every kernel instantiation of shade.hip stays within what profiles/shade_isa_resources.md recorded for it ("new" rows), in the
product build and in the knobs build: the same LDS and occupancy, no more scratch or registers, and no more v_*, ds_*, global_*,
s_waitcnt or s_barrier instructions in the cross-compiled gfx950 ISA (tools/isa_phase_count.py; scalar-ALU counts may move).  The
shade's kernels share their prologue pieces, and a piece that the compiler takes differently shows here in every kernel that uses
it.  Instruction classes are counted, no particular instruction is looked for.  No GPU; needs hipcc."""
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


@pytest.fixture(scope="module", params=[0, 1], ids=["product", "knobs"])
def tables(request):
    tool = load_tool()
    defines = tool.SHADE_BUILDS[request.param]
    now = {name: row for name, (row, _) in tool.kernel_table(tool.compile_isa(defines, tool.SRC)).items()}
    # the report holds one table per build, each under its own "# shade.hip ..." heading, in the order of SHADE_BUILDS
    sections = open(os.path.join(ROOT, "profiles", "shade_isa_resources.md")).read().split("# shade.hip")[1:]
    assert len(sections) == len(tool.SHADE_BUILDS)
    return tool, now, tool.parse_bloom_rows(sections[request.param], "new"), tool.parse_bloom_rows(sections[request.param], "parent")


def test_every_recorded_kernel_still_exists(tables):
    _, now, recorded, parent = tables
    assert len(recorded) == 21, "profiles/shade_isa_resources.md: each table lists 21 kernel instantiations"
    assert sorted(parent) == sorted(recorded), "one parent row and one new row per kernel"
    assert sorted(set(recorded) - set(now)) == []


def test_the_frame_kernels_are_in_the_table(tables):
    tool, _, recorded, _ = tables
    for k in (tool.PREFIX + "N3pbr7" + tool.FOLD_ARG[False], tool.PREFIX + "N3pbr7" + tool.FOLD_ARG[True], tool.TABLED_PREFIX, "k_shade_geometry_tables",
              "k_lut_fold_x", "k_env_pad", "10ShadeViews"):
        assert any(k in name for name in recorded), k


def test_the_recorded_rows_hold_the_condition_against_their_parent_rows(tables):
    tool, _, recorded, parent = tables
    assert {n: tool.exceeds(recorded[n], parent[n]) for n in recorded if tool.exceeds(recorded[n], parent[n])} == {}


def test_no_kernel_exceeds_its_recorded_row(tables):
    tool, now, recorded, _ = tables
    over = {}
    for name, ref in recorded.items():
        if name in now:
            print(name, now[name])
            bad = tool.exceeds(now[name], ref)
            if bad:
                over[name] = {c: (now[name][c], ref[c]) for c in bad}
    assert over == {}, f"(now, recorded) per column: {over}"
