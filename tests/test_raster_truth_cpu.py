"""The float64 truth of the rasterizer's interpolated attributes (tests/raster_truth.py) without a GPU: the numpy restatements
(raster_ref, raster_tex_ref: the reference the GPU's parity tests use) lie inside the truth's band on every case of
tests/test_gpu_raster_truth.py and under the caps on undecided and set-aside pixels; the truth agrees with exact rational arithmetic;
and the band rejects each of a list of defects injected into a copy of the truth evaluator."""
from fractions import Fraction

import numpy as np
import pytest

import raster_ref
import raster_tex_ref
import raster_truth as T
from raster_truth import Truth, vertex_attr

f32, f64 = np.float32, np.float64


@pytest.mark.parametrize("case", T.CASES, ids=repr)
def test_restatement_normals_inside_band(orc, case):
    """raster_ref's interpolated normal within the band of the truth, its B bytes among the admissible ones, and the case under
    both caps, for the three kinds of vertex normals"""
    _, _, ys, xs, t = case.geometry
    assert len(ys) >= 500
    if case.special:
        near, guard = case.special_wins()
        print(f"{case}: the near-plane triangle wins {near} pixels, the guard-band triangle {guard}")
        assert near >= T.SPECIAL_MIN and guard >= T.SPECIAL_MIN, (near, guard)
    tr, band = case.truth()
    un = band.units()
    print(f"{case}: barycentric band {np.median(un):.1f} u median, {un.max():.1f} u worst")
    for kind in T.NORMAL_KINDS:
        nv = T.vertex_normals(kind, len(case.positions) // 3, case.seed)
        v, i, d, _ = case.scene(normals=nv)
        taps = {}
        got = raster_ref.raster(case.g, case.tile, v, i, d, orc, taps=taps)
        assert np.array_equal(taps["ys"], ys) and np.array_equal(taps["t"], t)
        n, dn = band.here(vertex_attr(v["normal"], t))
        share = float((np.abs(taps["nrm"].astype(f64) - n) / dn).max())
        st = T.check_normal_bytes(got["B"][ys, xs], n, dn)
        print(T.describe(f"  {kind}: restatement uses {share:.3f} of the band", st))
        assert share <= 1.0 and st["bad"] == 0 and st["third"], (kind, share, st)
        assert T.within_caps(st), (kind, st)


@pytest.mark.parametrize("case", T.TEX_CASES, ids=repr)
def test_restatement_uv_lod_tangent_inside_band(orc, case):
    """raster_tex_ref's uv, LOD and tangent within the band at every step of texels per pixel, and the level it reads"""
    _, _, ys, xs, t = case.geometry
    tr, band = case.truth()
    tex = T.level_texture(T.LEVEL_REDS)
    tang = np.tile(np.eye(3), (len(case.positions) // 3, 1))
    worst = {"uv": 0.0, "lod": 0.0, "tan": 0.0}
    for k, half in T.TEX_STEPS:
        uvs = T.screen_uv(case, 2.0 ** (k + (0.5 if half else 0.0)))
        v, i, d, maps = case.scene(tangents=tang, uvs=uvs, maps={"roughness": 0})
        taps = {}
        got = raster_tex_ref.raster_textured(case.g, case.tile, v, i, d, maps, [tex], orc, taps=taps)
        uv, duv = band.here(vertex_attr(v["uv"], t))
        worst["uv"] = max(worst["uv"], float((np.abs(np.stack([taps["u"], taps["v"]], 1).astype(f64) - uv) / duv).max()))
        lod, dlod = band.lod(vertex_attr(v["uv"], t), T.TEX_SIZE, T.TEX_SIZE, tex["mips"])
        assert np.abs(tr.lod(vertex_attr(v["uv"], t), T.TEX_SIZE, T.TEX_SIZE, tex["mips"]) - lod).max() < 1e-12
        assert np.abs(lod - (k + (0.5 if half else 0.0))).max() < 1e-3, (k, half)          # the case is what it says
        ref_lod = raster_tex_ref.lod(tex, taps["dxu"], taps["dxv"], taps["dyu"], taps["dyv"]).astype(f64)
        worst["lod"] = max(worst["lod"], float((np.abs(ref_lod - lod) / dlod).max()))
        tg, dtg = band.here(vertex_attr(v["tangent"], t))
        worst["tan"] = max(worst["tan"], float((np.abs(taps["tan"].astype(f64) - tg) / dtg).max()))
        r = (got["C"][ys, xs] & 255).astype(f64)
        assert np.abs(r - T.expected_level_byte(T.LEVEL_REDS, k, half)).max() <= (0.5 if half else 0.0), (k, half, np.unique(r))
    print(f"{case}: restatement uses {worst} of the bands (LOD band {dlod.max():.2e} worst at the last step)")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("rgb", [T.TANGENT_RGB, T.TANGENT_RGB_565], ids=["decoded", "bc1"])
@pytest.mark.parametrize("case", T.TANGENT_CASES, ids=repr)
def test_restatement_tangent_readout(orc, case, rgb):
    """the normal-map frame on axis tangents, with the normal-map colour of the decoded and of the BC1-resident GPU instance:
    raster_tex_ref's B bytes are admissible, the case under both caps"""
    v, i, d, maps = T.tangent_scene(case)
    got = raster_tex_ref.raster_textured(case.g, case.tile, v, i, d, maps, [T.tangent_texture(rgb)], orc)
    _, _, ys, xs, _ = case.geometry
    st = T.check_tangent_bytes(case, got["B"][ys, xs], v, rgb)
    print(T.describe(f"{case} tangent", st))
    assert st["bad"] == 0 and st["third"] and T.within_caps(st), st


def test_truth_agrees_with_rational_arithmetic():
    """barycentrics of a handful of triangles and pixels (far corners of the largest frames among them) in exact fractions of the
    float32 clip coordinates: the float64 truth is within 1e-11 of them"""
    for name in ("256x144-origin-r4", "7680x4320-corner-r1.5", "8192x8192-corner-r12", "3840x2160-corner-r4-pitch_roll"):
        case = T.case(name)
        clip, _, ys, xs, t = case.geometry
        tr, _ = case.truth()
        b = tr.here(np.broadcast_to(np.eye(3), (len(t), 3, 3)))
        W, H = (Fraction(s) for s in case.full)
        for p in range(0, len(t), max(len(t) // 5, 1)):
            px, py = Fraction(2 * int(xs[p] + case.tile.x0) + 1, 2), Fraction(2 * int(ys[p] + case.tile.y0) + 1, 2)
            c = [[Fraction(float(a)) for a in vtx] for vtx in clip[t[p]]]
            X = [(v[0] + v[3]) * W / 2 - px * v[3] for v in c]
            Y = [(v[3] - v[1]) * H / 2 - py * v[3] for v in c]
            lam = [X[(i + 1) % 3] * Y[(i + 2) % 3] - Y[(i + 1) % 3] * X[(i + 2) % 3] for i in range(3)]
            exact = [float(l / sum(lam)) for l in lam]
            assert np.abs(b[p] - exact).max() <= 1e-11, (name, p, b[p], exact)


# ---- injected defects: each a copy of the truth evaluator with one step replaced
class ParentPlanes(Truth):
    """the planes formed in float32 from screen coordinates in pixels and evaluated at absolute pixel positions"""

    def edge(self, gx, gy):
        c = self.clip.astype(f32)
        sx, sy, sw = (c[..., 0] + c[..., 3]) * f32(self.half_w), (c[..., 3] - c[..., 1]) * f32(self.half_h), c[..., 3]
        (xj, xk), (yj, yk), (wj, wk) = T.cyc(sx), T.cyc(sy), T.cyc(sw)
        fx, fy = (np.asarray(gx).astype(f32) + f32(0.5))[:, None], (np.asarray(gy).astype(f32) + f32(0.5))[:, None]
        lam = ((yj * wk - wj * yk) * fx + (wj * xk - xj * wk) * fy) + (xj * yk - yj * xk)
        assert lam.dtype == f32
        return lam.astype(f64)


class OriginOffByOne(Truth):
    def centre(self, gx, gy):
        return gx + 1.5, gy + 0.5


class SwappedWeights(Truth):
    def weights(self, lam):
        return lam[:, [0, 2, 1]]


class ScreenLinear(Truth):
    def weights(self, lam):
        return lam * self.clip[..., 3]


class NoReciprocal(Truth):
    def normalise(self, num, total):
        return num


class DifferencesAtPixel(Truth):
    def quad(self):
        return (self.gx, self.gy), (self.gx + 1, self.gy), (self.gx, self.gy + 1)


def encoded_normal(orc, n):
    """B words of float64 normals [k, 3] through the oracle's encode"""
    m1 = np.zeros((1, len(n), 4), f32)
    m1[0, :, :3] = n.astype(f32)
    z = np.zeros((1, len(n), 4), f32)
    return orc.gbuffer_encode(z, m1, z)[1].reshape(-1)


def normal_verdict(orc, case, cls):
    """the byte rule's verdict on evaluator `cls` standing in for the kernel: axis normals read the barycentrics out"""
    _, _, ys, xs, t = case.geometry
    _, band = case.truth()
    attr = np.broadcast_to(np.eye(3), (len(t), 3, 3))
    n, dn = band.here(attr)
    return T.check_normal_bytes(encoded_normal(orc, case.truth(cls)[0].here(attr)), n, dn)


def test_the_sound_evaluator_passes(orc):
    for name in ("256x144-origin-r4", "1920x1080-corner-r4"):
        st = normal_verdict(orc, T.case(name), Truth)
        assert st["bad"] == 0 and T.within_caps(st), st


def test_parent_planes_are_rejected_from_1080p_up(orc):
    """the defect this band was made for: at 1920x1080 with 4-pixel triangles, its smallest appearance, and above.  At 256x144 the
    parent's planes are nearly inside the band, not inside it: their bytes differ from the truth's on under 1 % of the pixels and never
    by more than a step (the issue's measurement: 0.8 %, worst 1), so the rule may reject that many there and no more."""
    for name in ("1920x1080-corner-r4", "3840x2160-corner-r4", "7680x4320-corner-r4", "8192x8192-corner-r12"):
        st = normal_verdict(orc, T.case(name), ParentPlanes)
        print(T.describe(f"parent planes, {name}: {st['bad']} pixels rejected", st))
        assert st["bad"] > 0, (name, st)
    st = normal_verdict(orc, T.case("256x144-origin-r4"), ParentPlanes)
    print(T.describe(f"parent planes, control: {st['bad']} pixels rejected", st))
    assert st["bad"] <= 0.01 * st["pixels"], st


@pytest.mark.parametrize("cls", [OriginOffByOne, SwappedWeights, ScreenLinear], ids=lambda c: c.__name__)
def test_normal_defects_are_rejected(orc, cls):
    st = normal_verdict(orc, T.case("256x144-origin-r4"), cls)
    assert st["bad"] > 0.2 * st["pixels"], st


def test_uv_defects_are_rejected():
    """the dropped reciprocal (uv scaled by the sum of the edge functions) on the uv itself; differences taken from the pixel on the
    LOD, on a case with depth spread (on an affine field the two are the same differences)"""
    case = T.case("1920x1080-corner-r4")
    _, _, _, _, t = case.geometry
    tr, band = case.truth()
    uv = vertex_attr(T.screen_uv(case, 4.0), t)
    val, dval = band.here(uv)
    assert (np.abs(tr.here(uv) - val) <= dval).all()
    assert (np.abs(case.truth(NoReciprocal)[0].here(uv) - val) > dval).mean() > 0.9
    lod, dlod = band.lod(uv, T.TEX_SIZE, T.TEX_SIZE, 9)
    assert (np.abs(tr.lod(uv, T.TEX_SIZE, T.TEX_SIZE, 9) - lod) <= dlod).all()
    off = np.abs(case.truth(DifferencesAtPixel)[0].lod(uv, T.TEX_SIZE, T.TEX_SIZE, 9) - lod) > dlod
    odd = ((tr.gx | tr.gy) & 1) != 0        # (the quad's top-left pixel itself takes the same differences either way)
    assert off[odd].mean() > 0.9 and not off[~odd].any()


def test_level_blocks_hold_their_colours():
    """the BC1 chains of the GPU tests decode to their colours exactly"""
    import bc1_ref
    t = T.level_blocks(T.LEVEL_REDS_565)
    levels = bc1_ref.decode_chain(t["blocks"], t["width"], t["height"], t["mips"], t["format"])
    for l, (lv, r) in enumerate(zip(levels, T.LEVEL_REDS_565)):
        assert lv.shape[:2] == (T.TEX_SIZE >> l, T.TEX_SIZE >> l) and (lv[..., 0] == r).all() and not lv[..., 1:3].any(), l
    t = T.tangent_blocks()
    for lv in bc1_ref.decode_chain(t["blocks"], t["width"], t["height"], t["mips"], t["format"]):
        assert (lv[..., :3] == np.array(T.TANGENT_RGB_565, np.uint8)).all()
