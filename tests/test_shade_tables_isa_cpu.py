"""k_deferred_shade_tabled<257> (pbr_deferred_shade with tables) keeps the resources and the row body of the folded kernel it replaces
(profiles/shade_lut_fold_isa.md) and a prologue — the instructions outside its row loop, which a block runs once — no longer than
profiles/shade_tables_isa.md records and at most HALF the folded kernel's own, compiled in the same run: below that the tables have
lost their point.  No GPU; needs hipcc."""
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
    tabled = tool.measure(prefix=tool.TABLED_PREFIX)
    folded = tool.measure(fold=True)
    print("\n".join(tool.report(tabled, with_prologue=True)))
    print(f"folded kernel: prologue {folded['prologue']} v_*, {folded['prologue_barriers']} s_barrier")
    assert tabled["name"].startswith(tool.TABLED_PREFIX) and tool.FOLD_ARG[True] in folded["name"]
    fold_rec = tool.parse_metrics(open(os.path.join(ROOT, "profiles", "shade_lut_fold_isa.md")).read())
    recorded = tool.parse_metrics(open(os.path.join(ROOT, "profiles", "shade_tables_isa.md")).read())
    assert {"prologue", "prologue_barriers"} <= set(recorded), "profiles/shade_tables_isa.md: a prologue metric is missing"
    return tabled, folded, fold_rec, recorded


def test_resource_budget(counts):
    tabled = counts[0]
    assert tabled["occupancy"] == 5
    assert tabled["scratch"] == 0


def test_row_body_no_higher_than_the_folded_kernels_record(counts):
    tabled, _, fold_rec, _ = counts
    for key in ("hot_trip", "surround", "row_executed"):
        assert tabled[key] <= fold_rec[key], f"{key}: {tabled[key]:g} now, {fold_rec[key]:g} recorded for the folded kernel"


def test_prologue_no_higher_than_recorded(counts):
    tabled, _, _, recorded = counts
    assert tabled["prologue"] <= recorded["prologue"], f"prologue v_*: {tabled['prologue']} now, {recorded['prologue']:g} recorded"
    assert tabled["prologue_barriers"] <= recorded["prologue_barriers"]


def test_prologue_at_most_half_the_folded_kernels(counts):
    tabled, folded, _, _ = counts
    assert 2 * tabled["prologue"] <= folded["prologue"], f"prologue v_*: tabled {tabled['prologue']}, folded {folded['prologue']}"
    assert tabled["prologue_barriers"] < folded["prologue_barriers"]
