"""The sun light's rule on the CPU (tests/sun_truth.py): closed forms, the shadow's geometry against the analytic shadows of the
casters, pbr_sun_fit against its restatement and its stated margins, the set-aside cap of every GPU case, and nine injected
defects, each failing a named assertion.  No GPU.  `-s` prints the measured figures."""
import math

import numpy as np
import pytest

import camera_ref
import sun_cases as sc
import sun_truth as st
from direct12pbrrenderer_amd import _lib, api, scene
from direct12pbrrenderer_amd.structs import Tile

UNDECIDED_CAP, CLASS_FLOOR = 0.02, 0.05
GEOM = sc.Case("geometry-256x144-m64-pcf1", "default", 256, 144, 256, 64, 64, 64, 1)
GEOM3 = sc.Case("geometry-256x144-m64-pcf3", "default", 256, 144, 256, 64, 64, 64, 3)


def flat_gbuffer(w, h, nbytes, albedo_bytes, rough_byte, metal_byte, depth):
    """a G-buffer whose every pixel holds the same material, normal bytes and depth"""
    full = lambda v, dt: np.full((h, w), v, dtype=dt)
    return {"A": full(albedo_bytes[0] | albedo_bytes[1] << 8 | albedo_bytes[2] << 16 | 77 << 24, np.uint32),
            "B": full(nbytes[0] | nbytes[1] << 8, np.uint32), "C": full(rough_byte | metal_byte << 8, np.uint32),
            "depth": full(depth, np.float32), "stencil": full(1, np.uint8)}


def decoded_normal(nbytes):
    e = np.array(nbytes, dtype=np.float64) / 255.0
    d = np.array([e[0] * 2 - 1, e[1] * 2 - 1, 0.0])
    d[2] = 1.0 - abs(d[0]) - abs(d[1])
    assert d[2] >= 0
    return d / np.linalg.norm(d)


def test_closed_form_head_on_rough_dielectric():
    """vis = 1, N = L, roughness 1, metallic 0: NdotL = 1 kills the Fresnel term's power, a = 1 makes D = 1 / pi, k = 1 / 2, and
    c = (0.96 albedo / pi + 0.04 (1 / pi) G / max(4 NdotV, 1e-4)) E with G = NdotV / (NdotV / 2 + 1 / 2), written out by hand; the
    view vector comes from camera_ref's unprojection, not from the rule's own position."""
    w, h = 64, 36
    cam = scene.Camera.reference_default(w, h)
    g = scene.make_global(cam, w, h)
    tile = Tile(0, 0, w, h, w, h)
    nbytes, alb = (140, 150), (200, 120, 40)
    gb = flat_gbuffer(w, h, nbytes, alb, 255, 0, 0.99)
    n = decoded_normal(nbytes)
    sun = st.make_sun(n, (100.0, 90.0, 70.0))
    tr = st.truth(st.camera_of(g), tile, gb, sun)
    pos = camera_ref.unproject(g, tile, gb["depth"].astype(np.float64))
    v = np.array(g.CameraPos[:], dtype=np.float64) - pos
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    ndv = np.maximum(v @ n, 0.0)
    G = ndv / (ndv * 0.5 + 0.5)
    E = np.array([100.0, 90.0, 70.0])
    want = (0.96 * (np.array(alb) / 255.0) / st.PI64 + (0.04 / st.PI64 * G / np.maximum(4.0 * ndv, 1e-4))[..., None]) * E
    scale = want.max()
    # NdotL is 1 - O(1e-7) (the float32 direction): its effect on c is of that order; camera_ref's position differs from the rule's by
    # the float32 InvProjection / InvView of the constant buffer (1e-6 relative)
    assert np.abs(tr["contrib"] - want).max() <= 1e-5 * scale
    assert (ndv > 0.05).any() and tr["lit"].all()
    got = st.restate(st.camera_of(g), tile, gb, sun)
    assert np.abs(got[..., :3] - want).max() <= 1e-4 * scale and (got[..., 3] == 1).all()
    st.assert_probe(got, tr, got, "closed form")


def test_ndotl_not_positive_is_no_change():
    w, h = 32, 20
    g = scene.make_global(scene.Camera.reference_default(w, h), w, h)
    tile = Tile(0, 0, w, h, w, h)
    nbytes = (140, 150)
    gb = flat_gbuffer(w, h, nbytes, (200, 120, 40), 128, 30, 0.99)
    n = decoded_normal(nbytes)
    perp = np.cross(n, [0.0, 0.0, 1.0])
    for direction in (-n, -n + 0.3 * perp):
        sun = st.make_sun(direction, 100.0)
        assert not st.truth(st.camera_of(g), tile, gb, sun)["contrib"].any()
        assert not st.restate(st.camera_of(g), tile, gb, sun).any()


# ---- shadow geometry
def ground_tolerance(b, case, texels):
    """per pixel, in ground units: `texels` map texels (the diagonal, stretched by 1 / cos(TILT) where the tilted light meets the ground)
    plus one pixel's own footprint on the ground"""
    l, r, bb, t, n, f = b["ext"]
    texel = math.hypot((r - l) / case.map_w, (t - bb) / case.map_h) / math.cos(sc.TILT)
    is_ground, dist, pv = sc.ground_shadow_distance(b)
    step = np.maximum(np.linalg.norm(np.gradient(pv, axis=1), axis=-1), np.linalg.norm(np.gradient(pv, axis=0), axis=-1))
    return is_ground, dist, texels * texel + step


def test_shadow_matches_the_analytic_shadows(orc):
    """pcf 1: a ground pixel more than one texel (plus a pixel) inside a caster's analytic shadow has vis == 0, one that far outside
    every shadow has vis == 1: the four taps around the receiver lie within a texel of it, and the map's texel centres sample the
    casters exactly."""
    b = sc.build(GEOM, orc)
    is_ground, dist, tol = ground_tolerance(b, GEOM, 1.0)
    vis = b["truth"]["vis"]
    inside, outside = is_ground & (dist < -tol), is_ground & (dist > tol)
    assert inside.sum() > 500 and outside.sum() > 3000
    assert (vis[inside] == 0.0).all(), "a pixel deep inside the analytic shadow is not fully shadowed"
    assert (vis[outside] == 1.0).all(), "a pixel far outside every analytic shadow is not fully lit"
    assert ((vis == 0.0) & is_ground & b["truth"]["lit"]).sum() >= inside.sum()


def test_pcf3_penumbra_is_three_texels_wide(orc):
    """the 4 x 4 taps' nine footprints change while the shadow's edge passes three texel intervals; with the edge itself known to half
    a texel (the map samples the caster at texel centres) every penumbra pixel of the ground lies within 2 texels (plus a pixel) of an
    analytic edge"""
    b = sc.build(GEOM3, orc)
    is_ground, dist, tol = ground_tolerance(b, GEOM3, 2.0)
    vis = b["truth"]["vis"]
    pen = is_ground & (vis > 0.0) & (vis < 1.0)
    assert pen.sum() > 1000
    assert (np.abs(dist[pen]) <= tol[pen]).all(), "a penumbra pixel lies further than 2 texels from every analytic shadow edge"


def test_visibility_is_monotone_in_the_constant_bias(orc):
    b = sc.build(GEOM3, orc)
    prev = None
    for bias in (0.0, 0.01, 0.03, 0.1, 0.4, 1.5):
        sun = dict(b["sun"], bias_const=np.float32(bias))
        vis = st.truth(b["cam"], b["tile"], b["gb"], sun, b["depth_map"])["vis"]
        if prev is not None:
            assert (vis >= prev).all(), f"bias {bias}: a pixel got darker"
        prev = vis
    assert (prev[b["truth"]["lit"]] == 1.0).all()      # a bias beyond the depth range lights everything


def test_outside_the_map_and_outside_the_depth_range_is_lit(orc):
    b = sc.build(sc.BY_NAME["256x144-default-m16-pcf3"], orc)
    tr = b["truth"]
    q = tr["q"]
    su, sv = (q[..., 0] + 1) * 0.5 * 16 - 0.5, (1 - q[..., 1]) * 0.5 * 16 - 0.5
    off_map = tr["lit"] & ((su < -2) | (su >= 17) | (sv < -2) | (sv >= 17))
    assert off_map.sum() > 2000 and (tr["vis"][off_map] == 1.0).all()
    for shift in (2.0, -2.0):       # the whole scene beyond the far end / in front of the near end of the light's depth range
        M = b["sun"]["M"].copy()
        M[2, 3] += np.float32(shift)
        for fn in (lambda s: st.truth(b["cam"], b["tile"], b["gb"], s, b["depth_map"])["vis"],
                   lambda s: st.restate(b["cam"], b["tile"], b["gb"], s, b["depth_map"], details=(d := {})) is not None and d["vis"]):
            vis = fn(dict(b["sun"], M=M))
            assert (vis[tr["lit"]] == 1.0).all()


# ---- pbr_sun_fit
FIT_CASES = [((1.0, 1.0, 1.0), (-1.0, -2.0, -3.0), (4.0, 5.0, 6.0), 64, 40), ((0.0, 1.0, 0.0), (-3.0, 0.0, -3.0), (3.0, 2.0, 5.0), 16, 16),
             ((0.3, -0.9995, 0.01), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 2048, 2048), ((-0.5, 0.2, 0.8), (2.0, 2.0, 2.0), (2.0, 9.0, 2.5), 96, 3)]


@pytest.mark.parametrize("direction,mn,mx,mw,mh", FIT_CASES)
def test_sun_fit(direction, mn, mx, mw, mh):
    g, lvp = api.sun_fit(direction, mn, mx, mw, mh)
    V, P, IP, want_lvp, ext = st.sun_fit(direction, mn, mx, mw, mh)
    m4 = lambda a: np.array(a[:], dtype=np.float32).reshape(4, 4)
    assert np.array_equal(m4(g.View), V) and np.array_equal(m4(g.Projection), P) and np.array_equal(m4(g.InvProjection), IP)
    assert np.array_equal(m4(g.InvView), V.T) and np.array_equal(m4(lvp), want_lvp)
    assert tuple(g.Resolution[:]) == (float(mw), float(mh)) and g.Near == 0.0 and g.Far == 0.0 and g.Fov == 0.0
    assert tuple(lvp[12:]) == (0.0, 0.0, 0.0, 1.0)
    # the product of the stored matrices is LightViewProj; the stored inverses invert
    assert np.abs(m4(lvp).astype(np.float64) - P.astype(np.float64) @ V.astype(np.float64)).max() <= 2.0 ** -23 * np.abs(P).max()
    assert np.abs(P.astype(np.float64) @ IP.astype(np.float64) - np.eye(4)).max() <= 1e-5
    assert np.abs(V.astype(np.float64) @ V.T.astype(np.float64) - np.eye(4)).max() <= 1e-6
    # the view looks along -dir, left-handed: +z of the light's view is -dir, x cross y = z
    d = np.array(direction) / np.linalg.norm(direction)
    assert np.abs(V[2, :3] + d).max() <= 1e-6 and np.abs(np.cross(V[0, :3], V[1, :3]) - V[2, :3]).max() <= 1e-6
    alt = abs(d[1]) > 0.999
    up = np.array([1.0, 0.0, 0.0]) if alt else np.array([0.0, 1.0, 0.0])
    assert V[1, :3] @ up > 0 and abs(V[0, :3] @ up) <= 1e-6        # y leans towards `up`, x is perpendicular to it
    # the corners land inside the stated margins
    corners = np.array([[(mx if c & 1 else mn)[0], (mx if c & 2 else mn)[1], (mx if c & 4 else mn)[2], 1.0] for c in range(8)])
    q = corners @ m4(lvp).astype(np.float64).T
    slack = 1e-5
    assert np.abs(q[:, 0]).max() <= 1.0 - 2.0 / mw + slack and np.abs(q[:, 1]).max() <= 1.0 - 2.0 / mh + slack
    assert q[:, 2].min() >= 0.01 / 1.02 - slack and q[:, 2].max() <= 1.01 / 1.02 + slack
    # and tightly: the box's extreme corners sit on the margins (extents that were not replaced by the 1e-6 minimum)
    l, r, b, t, n, f = ext
    if r - l > 1e-3 and t - b > 1e-3 and f - n > 1e-3:
        assert abs(q[:, 0].max() - (1.0 - 2.0 / mw)) <= slack and abs(q[:, 0].min() + (1.0 - 2.0 / mw)) <= slack
        assert abs(q[:, 1].max() - (1.0 - 2.0 / mh)) <= slack and abs(q[:, 1].min() + (1.0 - 2.0 / mh)) <= slack
        assert abs(q[:, 2].min() - 0.01 / 1.02) <= slack and abs(q[:, 2].max() - 1.01 / 1.02) <= slack


def test_sun_fit_alternate_up():
    g, _ = api.sun_fit((0.0, 1.0, 0.0), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 32, 32)
    V = np.array(g.View[:]).reshape(4, 4)
    assert np.array_equal(V[2, :3], [0.0, -1.0, 0.0])            # looks straight down
    assert np.array_equal(np.abs(V[1, :3]), [1.0, 0.0, 0.0])     # y is the alternate up vector (1, 0, 0), not a division by zero
    assert np.isfinite(V).all()


def test_sun_fit_refusals():
    lib = _lib.load()
    for args in (((0.0, 0.0, 0.0), (0, 0, 0), (1, 1, 1), 16, 16), ((float("nan"), 1.0, 0.0), (0, 0, 0), (1, 1, 1), 16, 16),
                 ((0.0, 1.0, 0.0), (2, 0, 0), (1, 1, 1), 16, 16), ((0.0, 1.0, 0.0), (0, 0, 0), (1, float("inf"), 1), 16, 16),
                 ((0.0, 1.0, 0.0), (0, 0, 0), (1, 1, 1), 2, 16), ((0.0, 1.0, 0.0), (0, 0, 0), (1, 1, 1), 16, 8193)):
        with pytest.raises(api.PbrError):
            api.sun_fit(*args)
    assert lib.pbr_sun_fit(None, None, 16, 16, None, None) != 0


# ---- the set-aside cap and the classes of every GPU case, from the truth alone
@pytest.mark.parametrize("case", sc.CASES, ids=repr)
def test_set_aside_cap_and_classes(orc, case):
    b = sc.build(case, orc)
    cl = st.classes(b["truth"])
    print(f"{case.name}: {cl}")
    assert cl["undecided"] < UNDECIDED_CAP
    if case.shadows:
        for name in ("lit", "shadowed", "penumbra"):
            assert cl[name] >= CLASS_FLOOR, f"{name} pixels are {cl[name]:.3f} of the geometry"
    else:
        assert cl["lit"] + cl["undecided"] > 0.9
    # the restatement itself keeps the probe's bound (it is its own second term: this holds the bookkeeping, not the arithmetic)
    st.assert_probe(b["restated"], b["truth"], b["restated"], case.name)
    # and it is within 1e-4 of the pixel's scale of the truth on its own
    use = b["truth"]["lit"] & ~b["truth"]["undecided"]
    err = np.abs(b["restated"][use][:, :3] - b["truth"]["contrib"][use]).max(axis=-1) / b["truth"]["unshadowed"][use].max(axis=-1)
    print(f"{case.name}: float32 restatement within {err.max():.3g} of scale of the float64 truth")
    assert err.max() <= 1e-4


# ---- injected defects: each fails a named assertion
PROBE_DEFECTS = {"y_not_flipped": "256x144-pitch_roll-m96x40-pcf1", "half_dropped": "256x144-pitch_roll-m96x40-pcf1",
                 "bias_added": "256x144-default-m96x40-pcf3", "fresnel_ndotv": "256x144-default-noshadow",
                 "k_ibl": "70x45-pitch_roll-noshadow", "lum_permuted": "256x144-default-noshadow",
                 "ninth_sixteenth": "256x144-default-m96x40-pcf3", "outside_dark": "256x144-default-m16-pcf3"}


@pytest.mark.parametrize("defect", list(PROBE_DEFECTS))
def test_defect_misses_the_probe_bound(orc, defect):
    b = sc.build(sc.BY_NAME[PROBE_DEFECTS[defect]], orc)
    got = st.restate(b["cam"], b["tile"], b["gb"], b["sun"], b["depth_map"], defect=defect)
    with pytest.raises(AssertionError, match="probe bound missed"):
        st.assert_probe(got, b["truth"], b["restated"], defect)


def test_a_tie_is_lit_and_the_strict_comparison_is_caught(orc):
    """zr == stored is lit: a 1 x 1 map that stores one pixel's own zr lights that pixel; with `<` for `<=` it is dark"""
    b = sc.build(sc.BY_NAME["256x144-default-m96x40-pcf3"], orc)
    tie = sc.tie_case(b)
    sc.assert_tie_lit(lambda sun, depth_map: st.restate(b["cam"], b["tile"], b["gb"], sun, depth_map), tie)
    with pytest.raises(AssertionError, match="a tie is not lit"):
        sc.assert_tie_lit(lambda sun, depth_map: st.restate(b["cam"], b["tile"], b["gb"], sun, depth_map, defect="strict_less"), tie)


def test_defect_list_is_complete():
    assert set(PROBE_DEFECTS) | {"strict_less"} == set(st.DEFECTS) and len(st.DEFECTS) >= 8
