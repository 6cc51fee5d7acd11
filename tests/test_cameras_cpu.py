"""The CPU oracle under cameras that pitch and roll, against the float64 geometry of tests/camera_ref.py — and every precondition
the GPU tests of test_gpu_cameras.py rely on, so that a failure on the GPU is never a badly chosen input: the cameras really have
the matrix entries the default camera lacks, the light sets fill clusters to the cap and leave others empty, the world-position check
selects enough pixels over a wide range of distances, the shade cases are comparable and well-conditioned, the sky's checked
pixels are most of the frame."""
import numpy as np
import pytest

import camera_cases as cc
import camera_ref
import common
from direct12pbrrenderer_amd.structs import Tile
from shade_checks import F32_REL_LINF, _check_shade, _check_shade_f32, _truth_bound

BOX_RTOL, BOX_ATOL = 2e-6, 1e-7      # the suite's tolerance for cluster boxes (powf / tanf are libm-class)


@pytest.mark.parametrize("name", cc.NAMES)
def test_cameras_have_the_entries_the_default_lacks(name):
    cam, g = cc.make_global(name, 640, 360)
    inv = np.array(g.InvView[:], dtype=np.float64).reshape(4, 4)
    view = np.array(g.View[:], dtype=np.float64).reshape(4, 4)
    rot = inv[:3, :3]
    assert np.abs(rot @ rot.T - np.eye(3)).max() < 1e-6 and np.abs(view @ inv - np.eye(4)).max() < 1e-5
    assert np.array_equal(inv[:3, 3], np.array(g.CameraPos[:], dtype=np.float64))
    off = np.abs(rot.reshape(-1)[[1, 3, 5, 7]])
    nonzero = {"default": (), "roll_only": (1, 3), "pitch_only": (1, 5, 7), "pitch_roll": (1, 3, 5, 7)}[name]
    for k, v in zip((1, 3, 5, 7), off):
        assert (v > 0.02) if k in nonzero else (v < 1e-6), (k, v)
    if name == "default":   # the control is the reference's camera to the bit
        from direct12pbrrenderer_amd import scene
        assert cam.transform.tobytes() == scene.Camera.reference_default(640, 360).transform.tobytes() and float(g.Fov) == float(scene.f32(0.333) * scene.PI)
        assert np.abs(rot - np.diag([-1.0, 1.0, -1.0])).max() < 1e-6
    if name.startswith("pitch"):   # not its own transpose, and the x and z parts of InvView's column 1 — the shade's row term — count
        assert np.abs(rot - rot.T).max() > 0.2 and min(abs(rot[0, 1]), abs(rot[2, 1])) > 0.02


@pytest.mark.parametrize("frame", cc.BOX_FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("name", cc.NAMES)
def test_oracle_cluster_boxes_against_float64(orc, name, frame):
    cam, g = cc.make_global(name, *frame)
    got = orc.cluster_build(g)
    mn, mx = camera_ref.cluster_boxes(g)
    assert np.allclose(got["MinBound"], mn, rtol=BOX_RTOL, atol=BOX_ATOL) and np.allclose(got["MaxBound"], mx, rtol=BOX_RTOL, atol=BOX_ATOL)
    assert (mx > mn).all() and mn[:, 2].min() == pytest.approx(float(g.Near)) and mx[:, 2].max() == pytest.approx(float(g.Far))


@pytest.mark.parametrize("n", cc.CULL_LIGHTS)
@pytest.mark.parametrize("name", cc.NAMES)
def test_oracle_light_lists_against_float64_and_cull_preconditions(orc, name, n):
    cam, g = cc.make_global(name, *cc.CULL_FRAME)
    lights = cc.lights_around(n, cam)
    table = orc.cluster_build(g)
    boxes = (table["MinBound"].copy(), table["MaxBound"].copy())
    orc.cluster_cull(g, lights, table)
    lists, undecided = camera_ref.cull(g, lights, boxes, cc.CULL_MARGIN)
    assert undecided.mean() <= 0.02, f"{undecided.mean():.4f} of the clusters are undecided"
    got = camera_ref.lists_of_table(table)
    wrong = [c for c in np.flatnonzero(~undecided) if not np.array_equal(got[c], lists[c][:camera_ref.MAX_PER_CLUSTER])]
    assert not wrong, f"{len(wrong)} decided clusters differ from float64, first {wrong[0]}"
    assert table["NumLights"].max() == 32 and (table["NumLights"] == 0).any()
    pv = cc.view_space(g, lights["Position"])
    assert (pv[:, 2] < 0).any() and len(np.unique(lights["Radius"])) == 3 and len(np.unique(lights["Intensity"])) > n // 2
    seen = np.zeros(n, dtype=bool)
    seen[np.concatenate(lists)] = True
    assert 0.05 * n < (~seen).sum() < 0.5 * n, "some lights, not most, lie outside the frustum"
    print(f"[cameras] {name}, {n} lights: {undecided.mean() * 100:.2f} % of the clusters undecided, {int((~seen).sum())} lights reach no cluster")


@pytest.mark.parametrize("name", cc.NAMES)
def test_oracle_continues_a_partially_filled_list(orc, name):
    """a table whose every cluster starts at NumLights = 5 with five valid entries: the cull appends its hits from light 0 on"""
    cam, g = cc.make_global(name, *cc.CULL_FRAME)
    lights = cc.lights_around(300, cam)
    table = orc.cluster_build(g)
    lists, undecided = camera_ref.cull(g, lights, (table["MinBound"], table["MaxBound"]), cc.CULL_MARGIN)
    table["NumLights"] = 5
    table["LightIndex"][:, :5] = np.array([299, 0, 17, 17, 123])
    orc.cluster_cull(g, lights, table)
    for c in np.flatnonzero(~undecided):
        want = np.concatenate([[299, 0, 17, 17, 123], lists[c][:27]])
        assert table["NumLights"][c] == len(want) and np.array_equal(table["LightIndex"][c][:len(want)], want), c
    assert table["NumLights"].max() == 32 and table["NumLights"].min() == 5


def _shade32(orc, ibl, g, tile, gb, cl, lights):
    sky, env, lut, sh = ibl
    return orc.deferred_shade(g, tile, gb, lut, env, common.ENV_SIZE, common.ENV_MIPS, cl, lights, want_f32=True)[1]


@pytest.mark.parametrize("shape", cc.SHADE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", cc.NAMES)
def test_oracle_world_position_against_unproject(orc, ibl, name, shape):
    """(IA - I0) / (IB - I0) = 1 + 0.01 d^2 on the oracle's fp32 images, d from camera_ref.unproject(); and the selection the GPU test
    makes with the same inputs is large and spans a wide range of distances"""
    cam, g, _, gb, tile = cc.position_scene(name, shape, ibl[3])
    boxes = orc.cluster_build(g)
    none, every = cc.cluster_table(boxes, False), cc.cluster_table(boxes, True)
    pos = camera_ref.unproject(g, tile, gb["depth"])
    for p_view in cc.POSITION_LIGHTS_VIEW:
        la, lb = cc.position_light(g, p_view, 0.0), cc.position_light(g, p_view, cc.POSITION_C2)
        i0, ia, ib = (_shade32(orc, ibl, g, tile, gb, cl, l) for cl, l in ((none, la), (every, la), (every, lb)))
        sel, ratio, tol = cc.position_ratio(i0, ia, ib)
        d = np.linalg.norm(pos - la["Position"][0].astype(np.float64), axis=-1)
        want = 1.0 + cc.POSITION_C2 * d * d
        rel = np.abs(ratio - want) / want
        assert sel.sum() >= 200 and d[sel].max() >= 4.0 * d[sel].min(), (p_view, int(sel.sum()), d[sel].min(), d[sel].max())
        assert tol[sel].max() <= 0.05
        assert (rel[sel] <= tol[sel]).all(), f"light at {p_view}: relative error {rel[sel].max():.3g}"
        print(f"[cameras] {name} {shape[0]}x{shape[1]} light {p_view}: {int(sel.sum())} pixels, d {d[sel].min():.2f} .. {d[sel].max():.2f}, "
              f"oracle's worst relative error {rel[sel].max():.2g}")


@pytest.mark.parametrize("name", cc.NAMES)
def test_shade_cases_are_comparable_and_well_conditioned(orc, ibl, name):
    """the two conditions of the shade checks on every case of the GPU test — comparable pixels >= 0.95, well-conditioned >= 0.97 —
    and the oracle passes the fp32 check against itself (finite images, edge pixels, quantiles)"""
    for shape in cc.SHADE_SHAPES:
        for n in cc.SHADE_LIGHTS:
            for rough_min in cc.SHADE_ROUGH:
                c = cc.oracle_shade(orc, ibl, name, shape, n, rough_min)
                what = f"{name} {shape[0]}x{shape[1]}, {n} lights, rough_min {rough_min}"
                on = c["gb"]["stencil"] > 0
                _check_shade_f32(orc, c["want_f32"], c["want_f32"], c["truth"], c["gb"]["stencil"], what, rough=c["rough"])
                bound, scale, ok, d_orc = _truth_bound(orc, c["want_f32"], c["truth"], on, c["rough"])
                well = ok & (d_orc.max(axis=1) <= 0.25 * F32_REL_LINF * scale)
                assert ok.mean() >= 0.95 and well.mean() >= 0.97, (what, float(ok.mean()), float(well.mean()))
                if n == 1024:
                    assert c["cl"]["NumLights"].max() == 32 and len(c["lights"]) > 256


@pytest.mark.parametrize("name", cc.NAMES)
def test_folded_tile_case_passes_the_fp16_check_on_the_oracle(orc, ibl, name):
    """the 600 x 40 tile of a 4K frame the folded shade is held to the oracle on: the fp16 check's own conditions"""
    c = cc.oracle_shade(orc, ibl, name, cc.FOLD_TILE, cc.FOLD_LIGHTS, cc.FOLD_TILE_ROUGH_MIN)
    _check_shade(orc, c["want"], c["want"], c["want_f32"], c["truth"], c["gb"]["stencil"], f"{name} 600x40 tile", hard_ulp=None, rough=c["rough"])
    assert c["cl"]["NumLights"].max() == 32


@pytest.mark.parametrize("name", cc.NAMES)
def test_oracle_sky_holds_the_block_colours(orc, name):
    W, H = cc.SKY_FRAME
    cam, g = cc.make_global(name, W, H)
    tile = Tile(0, 0, W, H, W, H)
    sky = orc.cube_gen_mips(cc.block_sky(), cc.SKY_SIZE, cc.SKY_MIPS)
    hdr = np.full((H, W, 4), 3.0, np.float16)
    orc.skybox(g, tile, sky, cc.SKY_SIZE, cc.SKY_MIPS, np.zeros((H, W), np.uint8), hdr)
    want, inside = cc.sky_expectation(camera_ref, g, tile)
    assert 1.0 - inside.mean() <= 0.60, f"{1.0 - inside.mean():.3f} of the sky pixels are in the excluded margin"
    bad = (hdr[..., :3] != want).any(axis=-1) & inside
    assert not bad.any(), f"{int(bad.sum())} pixels hold another colour than their block's"
    assert len(np.unique(want[inside][:, 0])) >= 30 and (hdr[..., 3] == 1.0).all()
