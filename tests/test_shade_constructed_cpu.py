"""The constructed inputs of the shade (tests/shade_constructed.py), proved on the CPU before a GPU sees them: for every case the fp32
restatement alone passes the very checks the GPU image is put through; the inputs reach what the case table claims (kernel, light
stride, walk instantiation, all eight slices, every material byte, the list lengths, the slice and grid edges); and a wrong decision
would show — the restatement of the same inputs on cluster lists rolled by one cluster leaves the bound on most pixels of every slice.
These are conditions on the INPUTS: a light set that misses one is replaced by another seed of the grid, the condition stays."""
import numpy as np
import pytest

import shade_constructed as sc
from shade_checks import FLAG_CLUSTER_EDGE, MEASURED_TERM_CAP, _check_shade, _check_shade_f32

_MEASURED = {}


@pytest.fixture(params=sc.CASES, ids=[c.name for c in sc.CASES])
def built(request, orc):
    case = request.param
    b = sc.build(case, orc)
    if case.name not in _MEASURED:
        _MEASURED[case.name] = sc.measure(case, b, orc)
    return case, b, _MEASURED[case.name]


def test_the_restatement_passes_its_own_check(built, orc):
    case, b, m = built
    stencil = b["gb"]["stencil"]
    print(f"[constructed] {case.name}: restatement worst {m['worst']:.2e} of scale {m['scale']:.4g}, comparable {m['comparable']:.4f}, well-conditioned {m['well']:.4f}", flush=True)
    _check_shade_f32(orc, b["want_f32"], b["want_f32"], b["truth"], stencil, case.name, rough=b["rough"], decided=case.decided)
    assert m["comparable"] >= 0.95 and m["well"] >= 0.97, (m["comparable"], m["well"])
    finite = bool(np.isfinite(b["want"].astype(np.float32)).all())
    assert finite or case.rough_lo < 48, "a case of the bench's roughness range overflows half"
    if finite:
        _check_shade(orc, b["want"], b["want"], b["want_f32"], b["truth"], stencil, case.name, hard_ulp=None, rough=b["rough"], decided=case.decided)
    # the cap is in force exactly where the restatement itself is within it (rough-0 cases never take it)
    assert case.cap == (case.rough_lo >= 48 and max(m["worst"], m.get("worst_full", 0.0)) <= MEASURED_TERM_CAP), (case.cap, m["worst"], m.get("worst_full"))
    if case.staged:   # the tabled path shades the cull's own, untruncated table: the same checks on it
        want, want_f32, truth = sc.build_full(case, orc)
        print(f"[constructed] {case.name}, untruncated table: restatement worst {m['worst_full']:.2e} of scale, well-conditioned {m['well_full']:.4f}", flush=True)
        _check_shade_f32(orc, want_f32, want_f32, truth, stencil, case.name + " full", rough=b["rough"], decided=case.decided)
        assert np.isfinite(want.astype(np.float32)).all() or case.rough_lo < 48
        if np.isfinite(want.astype(np.float32)).all():
            _check_shade(orc, want, want, want_f32, truth, stencil, case.name + " full", hard_ulp=None, rough=b["rough"], decided=case.decided)
    if case.decided:   # ... and the keyword is what makes these cases comparable: without it the edge pixels are set aside
        on = stencil > 0
        assert ((b["truth"][2] & FLAG_CLUSTER_EDGE) != 0)[on].mean() > 0.04


def test_the_inputs_reach_what_the_case_table_claims(built, orc):
    case, b, m = built
    gb, lights, cl = b["gb"], b["lights"], b["clusters"]
    on = gb["stencil"] > 0
    assert 0.75 < on.mean() < 0.97 and on.sum() > 6000      # about a tenth of the 16 x 16 cells is stencilled off
    assert sc.dispatch(case) == (case.staged, case.stride) and len(lights) == case.n_lights
    assert sc.q_safe_of(lights) == case.q_safe
    waves = [t for row in sc.wave_t_ok(gb) for t in row if t is not None]
    assert len(waves) > 100 and all(t == case.t_ok for t in waves), "t_ok of a wave is not the case's"
    floor = 1000 if case.name.startswith("sweep-") or case.name == "unstaged" else 500
    assert (m["per_slice"] >= floor).all(), m["per_slice"]
    assert set(((gb["C"] >> 8) & 255)[on]) == set(range(256)), "metallic bytes"
    assert set((gb["C"] & 255)[on]) == set(range(case.rough_lo, 256)), "roughness bytes"
    assert len(set((gb["A"] >> 24)[on])) > 100 and 0.03 < ((gb["A"] >> 24)[on] > 0).mean() < 0.07, "emission bytes"
    nz = 1.0 - np.abs((gb["B"] & 255) / 255.0 * 2 - 1) - np.abs(((gb["B"] >> 8) & 255) / 255.0 * 2 - 1)
    assert 0.4 < (nz[on] < 0).mean() < 0.6, "the octahedral bytes fold on half of the pixels (back-facing normals among them)"
    used, lengths = m["used"], m["lengths"]
    assert {0, 1, 31, 32} <= lengths and any(n >= 3 and n % 2 for n in lengths) and len(lengths) >= 30, sorted(lengths)
    assert lengths & {3, 5} and lengths & {4, 8} and lengths & {7, 9}, "lengths on both sides of the walk's padding to four entries"
    k = np.arange(32)[None, :] < cl["NumLights"][:, None]
    assert cl["LightIndex"][k].min() >= 0 and cl["LightIndex"][k].max() < case.n_lights
    if case.n_lights > 256:
        assert cl["LightIndex"][used][k[used]].max() > 256, "no list of the tile indexes past the 257-stride table"
    assert sc.cull_margins(b["g"], lights, orc.cluster_build(b["g"])).min() >= sc.CULL_MARGIN, "a cull decision is within rounding of flipping"
    assert (b["clusters_full"]["NumLights"] >= cl["NumLights"]).all() and b["clusters_full"]["NumLights"].max() == 32
    if case.depth == "sweep":
        for d, want_slice in ((0.0, 0), (1.0, sc.CZ - 1)):   # the clamps at z = Near and z = Far
            at = on & (gb["depth"] == np.float32(d))
            assert at.sum() >= 3 and (m["sz"][at] == want_slice).all()
    if case.name == "slice-edges":
        depths, run = sc.slice_edge_depths(case.full, case.rect[2], orc)
        assert (np.diff(depths[:17].view(np.uint32).astype(np.int64)) == 1).all()
        for r in range(sc.CZ - 1):
            got = set(m["sz"][:, run == r][on[:, run == r]])
            assert got == {r, r + 1}, f"run {r}: slices {sorted(got)}"
    x0, y0, w, h = case.rect
    if case.name == "grid-edges":
        flags = b["truth"][2]
        cols = [x - x0 for x in sc.GRID_EDGE_COLUMNS]
        edge = np.zeros(on.shape, dtype=bool)
        edge[:, cols] = True
        edge[sc.GRID_EDGE_ROW - y0] = True
        assert ((flags[on & edge] & FLAG_CLUSTER_EDGE) != 0).all() and (on & edge).sum() > 300
        # ... and the fp32 column / row there is the upper cell's: the quotient rounds onto the integer
        assert [int(m["sx"][0, c]) for c in cols] == [1, 3, 5] and int(m["sy"][sc.GRID_EDGE_ROW - y0, 0]) == 9
        assert [int(m["sx"][0, c - 1]) for c in cols] == [0, 2, 4] and int(m["sy"][sc.GRID_EDGE_ROW - y0 + 1, 0]) == 8
    if case.name.startswith("sweep-4k"):
        assert sorted(set(m["sx"][0])) == [8, 9, 10, 11] and sorted(set(m["sy"][:, 0])) == [7, 8], "cluster columns at x = 1440, 1600, 1760, row edge at y = 1080"


def test_a_wrong_decision_would_show(built):
    case, b, m = built
    for k, rate in enumerate(m["catch"]["z"]):
        assert rate is not None and rate >= 0.80, f"lists rolled along z: caught on {rate} of slice {k}'s pixels ({m['catch']['z']})"
    print(f"[constructed] {case.name}: rolled lists caught on {min(m['catch']['z']):.3f} .. {max(m['catch']['z']):.3f} of a slice's pixels" +
          (f", x {m['catch']['x']:.3f}, y {m['catch']['y']:.3f} of the grid-edge pixels" if "x" in m["catch"] else ""), flush=True)
    if case.name == "grid-edges":
        assert m["catch"]["x"] >= 0.5 and m["catch"]["y"] >= 0.5, m["catch"]


def test_the_case_table_names_every_walk_and_both_kernels():
    walks = {(c.q_safe & 1, int(c.t_ok) if c.q_safe & 1 else 0, (c.q_safe >> 1) if c.q_safe & 1 else 0) for c in sc.CASES if c.staged}
    assert walks == {(1, 1, 1), (1, 1, 0), (1, 0, 1), (1, 0, 0), (0, 0, 0)}
    assert {c.staged for c in sc.CASES} == {True, False} and {c.stride for c in sc.CASES if c.staged} == {257, 1025}
