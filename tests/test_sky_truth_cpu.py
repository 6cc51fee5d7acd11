"""The float64 truth of the sky resolve (tests/sky_truth.py) validated without a GPU: the fp32 oracle's skybox passes the check on every
case of tests/sky_cases.py under the caps that keep the check from hiding a failure, the fp32 LOD lies within the derived tolerance T
of the float64 one (the table is printed), the truth reproduces the block-colour expectation of camera_cases, and check() rejects
six deliberately wrong resolves."""
import numpy as np
import pytest

import camera_cases
import camera_ref
import sky_cases as cases
import sky_truth as st
from direct12pbrrenderer_amd.structs import Tile

FLAG_CAP, WIDE_CAP, WIDE_CAP_ALL = 0.02, 0.05, 0.02
SENTINEL = 3.0


@pytest.fixture(scope="module")
def world(orc):
    """every case once: its inputs, cube, truth and the fp32 oracle's image (stencil and target with a pitch of w + 3 on the tile of a
    larger frame)"""
    cubes, out = {}, {}
    for case in cases.CASES:
        kind, size, mips, g, tile, stencil = cases.case_inputs(case)
        key = (kind, size, mips)
        if key not in cubes:
            cubes[key] = cases.make_cube(orc, kind, size, mips)
        pad = 3 if case[3][2] else 0
        sten = np.pad(stencil, ((0, 0), (0, pad)), constant_values=9)
        img = np.full((tile.h, tile.w + pad, 4), SENTINEL, np.float16)
        orc.skybox(g, tile, cubes[key], size, mips, sten, img)
        out[case] = dict(g=g, tile=tile, stencil=stencil, cube=cubes[key], size=size, mips=mips, image=img,
                         truth=st.truth(g, tile, sten, cubes[key], size, mips))
    return out


def test_the_fp32_oracle_passes_on_every_case(world):
    """check() on the oracle's image of every case; flagged pixels <= 2 % of a case's sky, pixels widened by an x.8 or LOD snap
    alternative <= 5 % of a case and <= 2 % of all; geometry and padding keep the sentinel, alpha is 1; and the inputs meet
    sky_cases.assert_coverage"""
    sky = wide = 0
    worst = {}
    for case, w in world.items():
        t, img = w["truth"], w["image"]
        n = len(t["iy"])
        assert n == int((w["stencil"] == 0).sum()) > 0, case
        r = st.assert_image(img, t, str(case))
        worst[case[:2]] = max(worst.get(case[:2], 0.0), r)
        assert (t["flag"] != 0).sum() <= FLAG_CAP * n, (case, int((t["flag"] != 0).sum()), n)
        assert t["wide"].sum() <= WIDE_CAP * n, (case, int(t["wide"].sum()), n)
        sky, wide = sky + n, wide + int(t["wide"].sum())
        keep = np.ones(img.shape[:2], bool)
        keep[t["iy"], t["ix"]] = False
        assert (img[keep] == SENTINEL).all() and (img[t["iy"], t["ix"], 3] == 1.0).all(), case
        if case[0] == "const":
            assert (img[t["iy"], t["ix"], :3] == np.float32(cases.CONST).astype(np.float16)).all() and img[t["iy"], t["ix"], 2].max() == 65504.0, case
    assert wide <= WIDE_CAP_ALL * sky, (wide, sky)
    print(f"\n[sky truth] {len(world)} cases, {sky} sky pixels, {wide} widened ({wide / sky:.4f}), fp32 oracle's worst pixel / bound by family:")
    for k, v in worst.items():
        print(f"[sky truth]   {k[0]:8s} {k[1][0]:3d}^2 x {k[1][1]}: {v:.3f}")
    cases.assert_coverage(cases.coverage({c: w["truth"] for c, w in world.items()}))


def test_fp32_lod_within_T_of_float64(world, orc):
    """|lod_f32 - lod_f64| <= T on every sky pixel of every case (no face tie, rho usable), and T is not idle: the largest ratio is at
    least 1 / 8.  The oracle itself is tied in through a level-coded cube, whose resolve IS its snapped LOD: it equals the truth's
    snapped LOD or its alternative on every pixel, and snap(clamp(lod_f32)) on all but 1e-3 of them (log2f's last place)."""
    table, seen = {}, set()
    for case, w in world.items():
        key = (case[1], case[2], case[3])
        if key in seen:
            continue
        seen.add(key)
        t, g, tile = w["truth"], w["g"], w["tile"]
        use = ~t["tie"] & (t["flag"] == 0)
        lf = st.lod_f32(g, tile, t)
        d = np.abs(lf.astype(np.float64) - t["lod"])[use]
        ratio = d / t["T"][use]
        assert (ratio <= 1.0).all(), (case, float(ratio.max()))
        row = table.setdefault(case[1], [0.0, 0.0, 0.0, 0])
        k = int(np.argmax(ratio))
        if ratio[k] > row[1]:
            row[1], row[2] = float(ratio[k]), float(t["T"][use][k])
        row[0], row[3] = max(row[0], float(d.max())), row[3] + int(use.sum())
        img = np.full((tile.h, tile.w, 4), SENTINEL, np.float16)
        orc.skybox(g, tile, cases.level_coded(w["size"], w["mips"]), w["size"], w["mips"], w["stencil"], img)
        got = img[t["iy"], t["ix"], 0].astype(np.float64)
        assert ((got == t["lod_s"]) | (got == t["lod_alt"]))[use].all(), case
        mine = np.floor(np.clip(np.nan_to_num(lf.astype(np.float64), nan=0.0), 0.0, w["mips"] - 1.0) * 256.0 + 0.5) / 256.0
        assert (got != mine)[use].sum() <= max(1, 1e-3 * use.sum()), (case, int((got != mine)[use].sum()))
    print("\n[sky truth] fp32 LOD against float64, per chain: pixels, max |d lod|, largest |d lod| / T and the T there")
    for chain, (dmax, rmax, t_at, n) in table.items():
        print(f"[sky truth]   {chain[0]:3d}^2 x {chain[1]}: {n:6d}  {dmax:.3e}  {rmax:.3f}  {t_at:.3e}")
    best = max(r[1] for r in table.values())
    assert 0.125 <= best <= 1.0, best


def test_fp32_lod_drift_grows_with_the_frame_and_stays_within_T(orc):
    """the cancellation in u_x - u_0 costs relative accuracy as a pixel gets smaller: the ragged tile at the centre and in the corner of
    640 x 360, 1920 x 1080 and 3840 x 2160 frames; |lod_f32 - lod_f64| <= T on every pixel, and the drift is printed per width"""
    w, h = cases.RAGGED[:2]
    cube = cases.make_cube(orc, "const", 4, 3)
    print("\n[sky truth] fp32 LOD drift by frame: camera, frame, tile origin, max |d lod|, largest |d lod| / T")
    worst = {}
    for W, H in ((640, 360), (1920, 1080), (3840, 2160)):
        for name in ("default", "pitch_roll"):
            g = cases.make_global(name, W, H)
            for x0, y0 in (((W - w) // 2, (H - h) // 2), (W - w, H - h)):
                tile = Tile(x0, y0, w, h, W, H)
                t = st.truth(g, tile, np.zeros((h, w), np.uint8), cube, 4, 3)
                d = np.abs(st.lod_f32(g, tile, t).astype(np.float64) - t["lod"])
                ratio = d / t["T"]
                assert (ratio <= 1.0).all(), (name, W, H, x0, y0, float(ratio.max()))
                worst[W] = max(worst.get(W, 0.0), float(d.max()))
                print(f"[sky truth]   {name:10s} {W:4d} x {H:4d} ({x0:4d}, {y0:4d}): {d.max():.3e}  {ratio.max():.3f}")
    assert worst[640] < worst[1920] < worst[3840] < 1.0 / 512.0      # it grows, and stays below half a LOD snap step at 4K


@pytest.mark.parametrize("name", camera_cases.NAMES)
def test_truth_reproduces_the_block_colour_expectation(orc, name):
    """camera_cases' sky of 384 one-colour blocks on the ragged tile of 640 x 360 (magnified: LOD 0): on the pixels a texel or more inside
    a block lo == hi == the block's colour, exactly"""
    w, h, (W, H), x0, y0 = cases.RAGGED
    _, g = camera_cases.make_global(name, W, H)
    tile = Tile(x0, y0, w, h, W, H)
    sky = orc.cube_gen_mips(camera_cases.block_sky(), camera_cases.SKY_SIZE, camera_cases.SKY_MIPS)
    t = st.truth(g, tile, np.zeros((h, w), np.uint8), sky, camera_cases.SKY_SIZE, camera_cases.SKY_MIPS)
    colour, inside = camera_cases.sky_expectation(camera_ref, g, tile)
    inside = inside.reshape(-1)
    assert inside.sum() > 2000 and (t["lod"] < 0).all()
    want = colour.reshape(-1, 3).astype(np.float64)[inside]
    assert np.array_equal(t["lo"][inside], want) and np.array_equal(t["hi"][inside], want)


def test_truth_rays_agree_with_the_unprojected_rays(world):
    """the truth's centre face is camera_ref's (rays through inv(Projection . View)) away from face ties"""
    for case, w in world.items():
        if case[2] == "diagonal":
            continue
        t = w["truth"]
        face, _, _ = camera_ref.cube_face_coords(camera_ref.ray_dirs(w["g"], w["tile"]), 1.0)
        assert (face[t["iy"], t["ix"]] == t["face"])[~t["tie"]].mean() >= 0.999, case


@pytest.mark.parametrize("mutation", st.MUTATIONS)
def test_check_rejects_a_wrong_resolve(world, mutation):
    """the image a resolve with one mistake would store — the truth code behind its test-only switch — fails check() on the case chosen
    for it, and the same image without the mistake passes"""
    case = cases.MUTATION_CASES[mutation]
    w = world[case]
    t = w["truth"]
    pad = w["image"].shape[1] - w["tile"].w
    sten = np.pad(w["stencil"], ((0, 0), (0, pad)), constant_values=9)
    wrong = st.truth(w["g"], w["tile"], sten, w["cube"], w["size"], w["mips"], mutation=mutation)
    ratio, ok = st.check(st.image_of(wrong, w["tile"].h, w["tile"].w), t)
    good, _ = st.check(st.image_of(t, w["tile"].h, w["tile"].w), t)
    print(f"\n[sky truth] {mutation}: {int((ratio[ok] > 1.0).sum())} of {int(ok.sum())} comparable pixels of {case} outside the bound, worst {ratio[ok].max():.3g} x")
    assert (good[ok] <= 1.0).all()
    assert (ratio[ok] > 1.0).sum() >= 4, mutation


def test_flags_mark_pixels_without_a_truth(orc):
    """an inf texel flags exactly the pixels whose footprint reaches it (FLAG_TAP) and the oracle's image still passes elsewhere"""
    case = ("checker", (4, 3), "pitch_roll", cases.A)
    kind, size, mips, g, tile, stencil = cases.case_inputs(case)
    cube = cases.make_cube(orc, kind, size, mips)
    face = int(np.bincount(st.truth(g, tile, stencil, cube, size, mips)["face"]).argmax())
    cube[(face * 4 + 1) * 4 + 1, 1] = np.inf          # texel (1, 1) of level 0 of the face most rays land on
    t = st.truth(g, tile, stencil, cube, size, mips)
    flagged = (t["flag"] & st.FLAG_TAP) != 0
    assert 0 < flagged.sum() < len(flagged) and (t["face"][flagged] == face).mean() > 0.5
    img = np.full((tile.h, tile.w, 4), SENTINEL, np.float16)
    orc.skybox(g, tile, cube, size, mips, stencil, img)
    st.assert_image(img, t, "inf texel")
    assert np.isfinite(img[t["iy"], t["ix"], :3].astype(np.float32)[~flagged]).all()
