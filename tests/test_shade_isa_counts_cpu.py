"""The instruction counts of k_deferred_shade<true, 257, false, NoViews> that tools/isa_phase_count.py reads from the cross-compiled
gfx950 ISA stay where profiles/shade_isa_counts_after.md recorded them: the kernel is bound by VALU issue, so an instruction that
creeps back into the walk or the row body is time, and so is a byte of scratch.  No GPU; needs hipcc."""
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
def counts():
    tool = load_tool()
    res = tool.measure()
    print("\n".join(tool.report(res)))
    recorded = tool.parse_metrics(open(os.path.join(ROOT, "profiles", "shade_isa_counts_after.md")).read())
    assert set(recorded) == {k for k, _ in tool.METRICS}, "profiles/shade_isa_counts_after.md: a metric is missing"
    return res, recorded


def test_resource_budget(counts):
    res, _ = counts
    assert res["occupancy"] == 5
    assert res["scratch"] <= 12


def test_every_walk_is_found_and_unrolled(counts):
    res, _ = counts
    # attenuation floor x GGX floor x shared polynomial: the five instantiations the kernel dispatches between
    assert len(res["walks"]) == 5
    for w in res["walks"]:
        assert w["unroll"] >= 2 and w["trans_per_trip"] == 4 and w["packed_per_trip"] >= 46, w


def test_counts_no_higher_than_recorded(counts):
    res, recorded = counts
    assert res["hot_trip"] <= 51
    for key in ("hot_trip", "surround", "row_executed"):
        assert res[key] <= recorded[key], f"{key}: {res[key]:g} now, {recorded[key]:g} recorded"
