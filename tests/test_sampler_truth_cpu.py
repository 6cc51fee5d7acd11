"""The float64 truth of the textured resolve's sampler (tests/sampler_truth.py) without a GPU: the numpy restatement
(raster_tex_ref.raster_textured, the reference of the GPU's parity tests) has no byte outside the truth's admissible ones on any
case, material, field and plane of tests/sampler_cases.py and stays under the caps; the inputs exercise what they are there for; the
truth agrees with exact rational arithmetic on the texel bytes; and the check rejects each of a list of defects injected into a copy
of the truth evaluator with one step replaced."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import raster_tex_ref
import raster_truth as T
import sampler_cases as C
import sampler_truth as S
from sampler_truth import Sampler

f64 = np.float64


@functools.lru_cache(maxsize=None)
def restatement(orc, case, mat, fld):
    v, i, d, maps = C.draw(case, mat, fld)
    return raster_tex_ref.raster_textured(case.g, case.tile, v, i, d, maps, [t.dict() for t in mat.table], orc)


@pytest.mark.parametrize("case", C.CASES, ids=repr)
@pytest.mark.parametrize("mat", C.MATERIALS, ids=repr)
def test_restatement_inside_truth(orc, case, mat):
    """every covered pixel's A, B and C bytes are admissible (B: but for the fold's set-aside), per field; the material's fields
    exercise the seam taps, both signs of uv, every level pair, f == 0 and both clamps"""
    C.assert_coverage(case, mat)
    worst = C.Worst()
    for fld in C.fields(mat, case):
        st = C.check(case, mat, fld, restatement(orc, case, mat, fld))
        worst.add(st)
        bad, ok = C.verdict(st)
        print(C.describe(f"  t {fld[0]:.4g} base {fld[1]}", st))
        assert bad == 0 and ok, (fld, st)
    print(f"{case} {mat}: restatement, {len(case.geometry[2])} pixels x {len(C.fields(mat, case))} fields, worst: {worst}")


@pytest.mark.parametrize("case", C.FLAT, ids=repr)
@pytest.mark.parametrize("mat", [m for m in C.MATERIALS if m.format != S.B8G8R8A8_SRGB], ids=repr)
def test_exact_field_reads_texel_bytes(orc, case, mat):
    """t = 1 with every pixel centre on a texel centre: every weight is 0 and unorm8(c / 255) == c, so C's bytes are the texels' red
    bytes, found here in integers on the level's own array, with no band involved; the truth's interval admits that byte alone"""
    _, _, ys, xs, _ = case.geometry
    want = C.exact_texel_bytes(case, mat.tex("surface"))
    got = restatement(orc, case, mat, C.EXACT)["C"][ys, xs].astype(np.int64)
    for shift in (0, 8, 16):
        assert np.array_equal((got >> shift) & 255, want), shift
    _, (lo, hi) = C.intervals(case, mat, C.EXACT, "surface")
    assert np.array_equal(T.unorm8(lo[:, 0]), want) and np.array_equal(T.unorm8(hi[:, 0]), want)
    assert len(np.unique(want)) > 100 or mat.bc1


def exact_sample(tex, u, v, lam):
    """the trilinear sample of one pixel in exact fractions of the texel bytes, on the level arrays (not the flat chain)"""
    u, v, lam = Fraction(float(u)), Fraction(float(v)), min(max(Fraction(float(lam)), Fraction(0)), Fraction(tex.mips - 1))
    l = lam.numerator // lam.denominator
    f = lam - l

    def texel(lv, x, y):
        if tex.format == S.R8:
            return [Fraction(int(lv[y, x]), 255), Fraction(0), Fraction(0)]
        return [Fraction(int(lv[y, x, k]), 255) for k in ((0, 1, 2) if tex.format == S.R8G8B8A8 else (2, 1, 0))]

    def bilinear(k):
        lv = tex.levels[k]
        h, w = lv.shape[:2]
        assert (w, h) == (tex.width >> k, tex.height >> k)
        x, y = u * w - Fraction(1, 2), v * h - Fraction(1, 2)
        x0, y0 = x.numerator // x.denominator, y.numerator // y.denominator
        fx, fy = x - x0, y - y0
        row = lambda yy: [(1 - fx) * a + fx * b for a, b in zip(texel(lv, x0 % w, yy % h), texel(lv, (x0 + 1) % w, yy % h))]
        return [(1 - fy) * a + fy * b for a, b in zip(row(y0), row(y0 + 1))]

    return [float((1 - f) * a + f * b) for a, b in zip(bilinear(l), bilinear(min(l + 1, tex.mips - 1)))]


def test_truth_agrees_with_rational_arithmetic():
    """on a handful of pixels of a non-square, an odd-sized, a partial and a BC1-resident chain: within 1e-12"""
    for name, case, fld in (("noise-64x16xfull-f28", C.CASES[0], (2.0 ** 0.5, C.BASE)), ("noise-37x21xfull-f61", C.CASES[2], (3.3, C.BASE)),
                            ("noise-16x64xfull-f87", C.CASES[1], (0.37, C.BASE)), ("noise-64x64x3-f28", C.CASES[2], (3.3, C.BASE)),
                            ("bc1-32x32x6-f28", C.CASES[1], (11.0, C.BASE))):
        mat = C.material(name)
        tex = mat.tex("surface")
        (u, _, v, _, lam, _), _ = C.pixels(case, mat, fld)
        got = tex.sampler().sample(u, v, lam)
        for p in range(0, len(u), max(len(u) // 6, 1)):
            want = exact_sample(tex, u[p], v[p], lam[p])
            assert np.abs(got[p] - want).max() <= 1e-12, (name, p, got[p], want)


# ---- injected defects: each a copy of the truth evaluator with one step replaced
class NoHalfTexel(Sampler):
    def coords(self, u, v, l):
        w, h = self.size(l)
        return u * w, v * h


class ClampedTaps(Sampler):
    def taps(self, x, n):
        fl = np.floor(x)
        i = fl.astype(np.int64)
        return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), x - fl


class SeamTapUnwrapped(Sampler):
    lenient = True

    def taps(self, x, n):
        x0, _, f = super().taps(x, n)
        return x0, x0 + 1, f


class FlippedV(Sampler):
    def coords(self, u, v, l):
        return super().coords(u, 1.0 - v, l)


class CurveAfterFilter(Sampler):
    def decode(self, c):
        return c / 255.0

    def resolve(self, s):
        return self.curve(s) if self.curved() else s


class CurveOn87(Sampler):
    def curved(self):
        return self.fmt in (S.B8G8R8A8, S.B8G8R8A8_SRGB)


class CurveWithheld(Sampler):
    def curved(self):
        return False


class RedBlueSwapped(Sampler):
    def red_first(self):
        return not super().red_first()


class LevelWeightsExchanged(Sampler):
    def blend(self, a, b, f):
        return f * a + (1.0 - f) * b


class NearestLevel(Sampler):
    def blend(self, a, b, f):
        return np.where(f < 0.5, a, b)


class WidthFromHeight(Sampler):
    lenient = True

    def size(self, l):
        return self.height >> l, self.height >> l


class CeilSizes(Sampler):
    lenient = True

    def size(self, l):
        return -((-self.width) >> l), -((-self.height) >> l)


class GreyR8(Sampler):
    def r8(self, r):
        return np.stack([r, r, r], axis=-1)


class CurveForGamma(Sampler):
    def gamma(self, s):
        return self.curve(s)


class UpperLevelUnclamped(Sampler):
    """l + 1 is not clamped (levels past the chain's end wrap into it)"""
    lenient = True

    def pair(self, lam):
        l = np.floor(lam).astype(np.int64)
        return l, l + 1, lam - l


class PastTheChain(UpperLevelUnclamped):
    """... and lambda is not clamped above either: l and l + 1 run past the partial chain's last level"""

    def clamp(self, lam):
        return np.maximum(lam, 0.0)


class SumOfDifferences(T.Truth):
    def footprint(self, ddx, ddy, tex_w, tex_h):
        size = np.array([tex_w, tex_h], f64)
        return np.hypot(*(ddx * size).T) + np.hypot(*(ddy * size).T)


class WidthOnBothAxes(T.Truth):
    def footprint(self, ddx, ddy, tex_w, tex_h):
        return super().footprint(ddx, ddy, tex_w, tex_w)


SRGB, WIDE, TALL, ODD, PARTIAL, BC1 = (m.name for m in (C.MATERIALS[0], C.MATERIALS[1], C.MATERIALS[2], C.MATERIALS[3], C.MATERIALS[4],
                                                      C.MATERIALS[6]))
ROOT2 = 2.0 ** 0.5
# (the defect, the case that catches it: case index, material, t of the field from BASE, the role whose plane shows it)
DEFECTS = [
    (NoHalfTexel, 0, WIDE, 0.37, "surface"),
    (ClampedTaps, 1, TALL, 0.37, "surface"),                # u < 0 on the whole tile: every tap would be texel 0
    (SeamTapUnwrapped, 0, ODD, 0.37, "surface"),            # the tile crosses u = -2 and v = 0: the pixels along those two lines
    (FlippedV, 2, WIDE, 1.0, "surface"),
    (CurveAfterFilter, 0, SRGB, 0.37, "surface"),           # magnified: every pixel interpolates between distant values
    (CurveOn87, 1, TALL, ROOT2, "surface"),
    (CurveWithheld, 1, SRGB, ROOT2, "albedo"),
    (RedBlueSwapped, 0, WIDE, 1.0, "surface"),
    (RedBlueSwapped, 2, BC1, 1.0, "surface"),
    (LevelWeightsExchanged, 0, PARTIAL, 3.3, "surface"),    # f = 0.72
    (NearestLevel, 1, WIDE, 3.3, "surface"),                # f = 0.72 (at 2^(1/2) the box straddles the defect's own jump at f = 1/2)
    (WidthFromHeight, 0, WIDE, 3.3, "surface"),
    (WidthFromHeight, 0, TALL, 3.3, "surface"),
    (CeilSizes, 2, ODD, 3.3, "surface"),                    # 37 >> 1 = 18, not 19
    (GreyR8, 1, ODD, ROOT2, "normal"),
    (CurveForGamma, 0, WIDE, 1.0, "albedo"),
    (PastTheChain, 0, PARTIAL, 11.0, "surface"),
    (SumOfDifferences, 2, TALL, ROOT2, "surface"),
    (WidthOnBothAxes, 1, WIDE, ROOT2, "surface"),           # the y difference is scaled by 64, not 16: lambda + 2
]


@pytest.mark.parametrize("defect,case,name,t,role", DEFECTS, ids=lambda x: x.__name__ if isinstance(x, type) else None)
def test_defect_is_rejected(orc, defect, case, name, t, role):
    """the restatement's bytes, admissible under the sound truth on this input (test_restatement_inside_truth), are not under the
    truth with the defect: more than a fifth of the pixels fail (of a defect at the seam: more than a fifth of the pixels whose
    footprint lies across it, one pixel in twelve at this magnification)"""
    case, mat, fld = C.CASES[case], C.material(name), (t, C.BASE)
    kind = {"truth": defect} if issubclass(defect, T.Truth) else {"sampler": defect}
    planes = restatement(orc, case, mat, fld)
    sound = C.check(case, mat, fld, planes, roles=(role,))[C.PLANE_OF[role]]
    st = C.check(case, mat, fld, planes, roles=(role,), **kind)[C.PLANE_OF[role]]
    print(f"{defect.__name__} on {case} {mat} t {t:.4g}: {st['bad']} of {st['pixels']} pixels rejected on {C.PLANE_OF[role]}")
    share = 0.2 / 12 if defect is SeamTapUnwrapped else 0.2
    assert sound["bad"] == 0 and st["bad"] > share * st["pixels"], (sound, st)


def test_unclamped_upper_level_has_weight_zero(orc):
    """min(l + 1, mips - 1) binds only where lambda == mips - 1, and there f == 0: the level it keeps the sampler from reading
    does not contribute (the kernel does not read it at all).  Dropping that clamp alone therefore changes no value, and no check
    of values can reject it; what a check can see is lambda's own upper clamp, whose loss takes l and l + 1 past the partial chain's
    end (PastTheChain in DEFECTS)."""
    case, mat = C.CASES[0], C.material(PARTIAL)
    tex = mat.tex("surface")
    for t in (3.3, 11.0):
        (u, _, v, _, lam, _), _ = C.pixels(case, mat, (t, C.BASE))
        sound, defect = tex.sampler(), tex.sampler(UpperLevelUnclamped)
        l0, l1, f = defect.pair(defect.clamp(lam))
        assert ((l1 <= tex.mips - 1) | (f == 0)).all() and (t < 11.0 or (l1 == tex.mips).all())
        assert np.array_equal(sound.sample(u, v, lam), defect.sample(u, v, lam))
