"""The folded-LUT instantiation k_deferred_shade<true, 257, false, NoViews, true> (pbr_deferred_shade with lut_fold) keeps the resources and
the walk of the sampled one and stays at the instruction counts profiles/shade_lut_fold_isa.md records for its row body and its LUT
phase; the row body is below the sampled kernel's recorded count (profiles/shade_isa_counts_after.md) — that difference is what the
table is for.  No GPU; needs hipcc."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def counts():
    spec = importlib.util.spec_from_file_location("isa_phase_count", os.path.join(ROOT, "tools", "isa_phase_count.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    res = tool.measure(fold=True, lut_phase=True)
    print("\n".join(tool.report(res)))
    assert tool.FOLD_ARG[True] in res["name"], res["name"]
    sampled = tool.parse_metrics(open(os.path.join(ROOT, "profiles", "shade_isa_counts_after.md")).read())
    recorded = tool.parse_metrics(open(os.path.join(ROOT, "profiles", "shade_lut_fold_isa.md")).read())
    assert set(recorded) == {k for k, _ in tool.METRICS + [tool.LUT_METRIC]}, "profiles/shade_lut_fold_isa.md: a metric is missing"
    return res, sampled, recorded


def test_resource_budget(counts):
    res, _, _ = counts
    assert res["occupancy"] == 5
    assert res["scratch"] == 0


def test_walks_as_in_the_sampled_kernel(counts):
    res, sampled, _ = counts
    assert len(res["walks"]) == 5
    for w in res["walks"]:
        assert w["unroll"] >= 2 and w["trans_per_trip"] == 4 and w["packed_per_trip"] >= 46, w
    assert res["hot_trip"] <= sampled["hot_trip"]


def test_counts_no_higher_than_recorded(counts):
    res, sampled, recorded = counts
    for key in ("hot_trip", "surround", "row_executed", "lut_phase"):
        assert res[key] <= recorded[key], f"{key}: {res[key]:g} now, {recorded[key]:g} recorded"
    # the x side of the sample is ~30 instructions: a folded kernel that is not at least 25 below the sampled one has lost the point
    assert res["surround"] <= sampled["surround"] - 25, f"surround {res['surround']:g}, sampled {sampled['surround']:g}"
