"""float64 truth for the material sampler of the G-buffer rasterizer's textured resolve (gbuffer_raster.hip: wrap_texel, texel,
taps_bc1, bilinear, sample) and for the map branches that feed the encode, the interval of admissible values per pixel, and the byte
rules on the A, B and C planes.  Written from the header's text (include/pbr_hip.h, "The sampler (SamplerLinearWrap ...), pinned"
and pbr_texture2d's layout), not from the kernel and not from tests/raster_tex_ref.py: that file restates the kernel lerp for lerp, so
a mistake made in both passes their comparison.  tests/test_sampler_truth_cpu.py holds the restatement to this truth and shows that
each of a list of defects is rejected; tests/test_gpu_sampler_truth.py holds the kernel to it.  Of raster_truth this module uses the
unit roundoff, unorm8 and the normal's rule (mapped_normal, check_normal_bytes); of bc1_ref the decode of a BC1 chain.

The statement.  A chain is the bytes of pbr_texture2d: level l is (width >> l) x (height >> l) texels, rows tightly packed, levels
concatenated from level 0 (Sampler reads the flat bytes, so the layout is part of the truth).
  Decode, before filtering   UNORM8 c -> c / 255; the sRGB curve on the colour bytes of format 91 only; .x is red for every format
                             (28 stores R, G, B, A; 87 and 91 store B, G, R, A); R8 reads as (r, 0, 0).
  Level                      lambda clamped to [0, mips - 1]; l = floor(lambda), f = lambda - l; levels l and min(l + 1, mips - 1),
                             blended (1 - f) : f.  lambda itself is raster_truth.Truth.lod's, unclamped.
  Bilinear                   texel coordinates (u w_l - 1/2, v h_l - 1/2), floor and fraction, both taps wrapped by non-negative
                             modulo, the plain convex combination.
  Maps                       roughness, metallic, AO = sample.x; albedo = sample.rgb ** 2.2; normal = ts.x t + ts.y b + ts.z n with
                             ts = 2 sample.rgb - 1 (raster_truth.mapped_normal).

The interval.  The sample S(u, v, lambda) is continuous: bilinear interpolation is continuous across texel lines (the tap that leaves
has weight 0 there) and across the wrap (the texture is periodic), the level blend is continuous at integer lambda (the level that
leaves has weight 0) and constant beyond the clamps.  So no pixel is set aside.  The kernel's (u, v, lambda) lie in the box
(u +- du, v +- dv, lambda +- dlambda) of raster_truth.Band (here, lod with clamp=False; the two ends of lambda are clamped, not the
centre, so that under magnification the interval does not widen for nothing), and [lo, hi] is the exact range of S over that box:
  * texel lines of the levels in play and integer lambda cut the box into pieces; on a piece the four taps of either level and the
    level pair are fixed, so S is affine in each of u, v and lambda with the other two held (a bilinear patch blended by f): a
    function affine in each variable takes its extremes over a box at the box's corners;
  * the box is narrower than one texel of its finest level and one unit of lambda (asserted), so every axis is cut at most once per
    level: the piece corners are the points of {lo, hi, the line of level l, of l + 1, of l + 2} in u, the same in v, times
    {lo, hi, the integer} in lambda, with l = floor(lambda_lo) (beyond an integer lambda the pair is (l + 1, l + 2)); where an axis has
    no line inside the box its midpoint stands in (a point of the box: it cannot widen the range).  The minimum and maximum are
    attained, so the range is exact, not an outer bound.  A box that no line and no integer cuts (nearly all) takes its 8 corners
    and its centre; the others take the whole 5 x 5 x 3 grid as well.
The kernel's own float32 steps then widen it:
  * the texel coordinate fl(fl(u w_l) - 1/2): at most u32 |u w_l| + u32 |u w_l - 1/2| texels, u32 = 2^-24, that is
    u32 (2 |u| + 1/2) in u for any w_l >= 1: added to du (dv likewise) before the box is formed.  The fraction x - floor(x) and
    lambda - floor(lambda) are exact in float32;
  * on the value, SAMPLER_STEPS = 10 u32: the table entry's rounding (1) and three nested lerps fmaf(b, f, a (1 - f)) of values in
    [0, 1], each the rounding of 1 - f, of the product and of the fmaf (3 x 3); a convex combination does not amplify what it is given;
  * the encode's unorm8, fl(fl(255 x) + 1/2): ENCODE_STEPS = 3 u32 (the product's u32 x, the sum's u32 256 / 255, rounded up).

The byte rule is raster_truth.check_normal_bytes's on all three planes: the admissible bytes are floor(255 v + 1/2) at both ends
of the interval, and every byte between.
  C  the interval of sample.x, directly.
  A  s ** 2.2 at both ends (monotone on [0, 1]), widened by the band of exp2(2.2 log2 c) as gbuffer_encode.hpp states it, 1 ULP
     (2^-23 relative) for each of the two transcendental instructions and 2^-24 for the product:
     relative ln 2 . 2.2 |log2 c| (2^-23 + 2^-24) + 2^-23.  The 1 ULP figure is that comment's claim; albedo_stats reports the largest
     multiple of this band any byte needs (trans), so that a wrong figure shows as trans > 1.  (A byte needs it only where
     255 s ** 2.2 comes within 4e-5 of a rounding boundary from outside an interval that the uv band has already made a thousand
     times as wide: trans == 0 on every input so far says that nothing contradicts the figure, not that it was confirmed.)
  B  ts = 2 s - 1 with the band (hi - lo) + u32 about the interval's middle, through mapped_normal, octahedral and check_normal_bytes;
     the only pixels set aside are the fold's sign decisions, theirs."""
import numpy as np

import bc1_ref
from raster_truth import U, check_normal_bytes, mapped_normal, unorm8

f64 = np.float64
R8G8B8A8, B8G8R8A8, B8G8R8A8_SRGB, R8 = 28, 87, 91, 61          # the DXGI numbers (include/pbr_hip.h, PBR_TEX_*)
assert set(bc1_ref.STORED) == {R8G8B8A8, B8G8R8A8, B8G8R8A8_SRGB, R8}
SAMPLER_STEPS, ENCODE_STEPS = 10, 3
UNDECIDED_CAP = 0.10


class Sampler:
    """The float64 sampler of one chain: data (the chain's bytes in pbr_texture2d's layout), width, height, mips, fmt.  The steps are
    methods so that a test can replace exactly one of them with a defect (lenient: a defect may index past the chain; it wraps)."""
    lenient = False

    def __init__(self, data, width, height, mips, fmt):
        self.data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        self.width, self.height, self.mips, self.fmt = int(width), int(height), int(mips), int(fmt)

    # ---- the chain
    def size(self, l):
        return self.width >> l, self.height >> l

    def offset(self, l):
        """texels in front of level l [k]"""
        l = np.asarray(l, dtype=np.int64)
        out = np.zeros(l.shape, np.int64)
        for i in range(int(l.max()) if l.size else 0):
            w, h = self.size(i)
            out += np.where(l > i, w * h, 0)
        return out

    # ---- decode, before the filter
    def red_first(self):
        return self.fmt == R8G8B8A8

    def curved(self):
        return self.fmt == B8G8R8A8_SRGB

    def r8(self, r):
        z = np.zeros_like(r)
        return np.stack([r, z, z], axis=-1)

    def stored_rgb(self, idx):
        """the (r, g, b) bytes [k, 3] of texels idx (texel numbers from the chain's start)"""
        texels = self.data if self.fmt == R8 else self.data.reshape(-1, 4)
        assert self.lenient or ((idx >= 0) & (idx < len(texels))).all()
        got = np.take(texels, idx, axis=0, mode="wrap").astype(np.int64)
        if self.fmt == R8:
            return self.r8(got)
        return got[:, [0, 1, 2] if self.red_first() else [2, 1, 0]]

    def curve(self, x):
        return np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)

    def decode(self, c):
        x = c / 255.0
        return self.curve(x) if self.curved() else x

    def resolve(self, s):
        """what is done to the filtered value: nothing"""
        return s

    # ---- bilinear
    def coords(self, u, v, l):
        w, h = self.size(l)
        return u * w - 0.5, v * h - 0.5

    def taps(self, x, n):
        """(tap 0, tap 1, fraction) of texel coordinate x on a level of n texels"""
        fl = np.floor(x)
        i = fl.astype(np.int64)
        n = np.maximum(n, 1)
        return np.mod(i, n), np.mod(i + 1, n), x - fl

    def fetch(self, l, x, y):
        w, _ = self.size(l)
        return self.decode(self.stored_rgb(self.offset(l) + y * w + x))

    def bilinear(self, l, u, v):
        w, h = self.size(l)
        x, y = self.coords(u, v, l)
        x0, x1, fx = self.taps(x, w)
        y0, y1, fy = self.taps(y, h)
        fx, fy = fx[:, None], fy[:, None]
        top = (1.0 - fx) * self.fetch(l, x0, y0) + fx * self.fetch(l, x1, y0)
        bottom = (1.0 - fx) * self.fetch(l, x0, y1) + fx * self.fetch(l, x1, y1)
        return (1.0 - fy) * top + fy * bottom

    # ---- the levels
    def clamp(self, lam):
        return np.clip(lam, 0.0, self.mips - 1.0)

    def pair(self, lam):
        """(l, the level above, f) of a clamped lambda"""
        l = np.floor(lam).astype(np.int64)
        return l, np.minimum(l + 1, self.mips - 1), lam - l

    def blend(self, a, b, f):
        return (1.0 - f) * a + f * b

    def sample(self, u, v, lam):
        """[k, 3] at uv with the (unclamped) lambda"""
        l0, l1, f = self.pair(self.clamp(np.asarray(lam, f64)))
        return self.resolve(self.blend(self.bilinear(l0, u, v), self.bilinear(l1, u, v), f[:, None]))

    # ---- the albedo branch
    def gamma(self, s):
        return s ** 2.2


def bc1_sampler(blocks, width, height, mips, fmt, cls=Sampler):
    """the sampler of a BC1-resident chain: the chain pbr_bc1_decode would produce (bc1_ref, held to known answers)"""
    levels = bc1_ref.decode_chain(blocks, width, height, mips, fmt)
    return cls(np.concatenate([np.ascontiguousarray(l).reshape(-1) for l in levels]), width, height, mips, fmt)


def interval(smp, u, du, v, dv, lam, dlam):
    """[lo, hi] [k, 3]: the range of the sample over the box (module docstring) plus the sampler's float32 steps; u, v, lam [k] the
    truth's (lam unclamped), du, dv, dlam raster_truth.Band's"""
    du, dv = du + U * (2.0 * np.abs(u) + 0.5), dv + U * (2.0 * np.abs(v) + 0.5)
    llo, lhi = smp.clamp(lam - dlam), smp.clamp(lam + dlam)
    assert np.isfinite(dlam).all() and (lhi - llo < 1.0).all(), "the lambda box spans more than one integer"
    l0 = np.floor(llo).astype(np.int64)

    def cuts(lo, hi, axis):
        """the lines of levels l0, l0 + 1, l0 + 2 inside (lo, hi), the midpoint where there is none, and whether there is any"""
        out, mid, cut = [], 0.5 * (lo + hi), np.zeros(len(lo), bool)
        for j in range(3):
            n = np.maximum(np.asarray(smp.size(np.minimum(l0 + j, smp.mips - 1))[axis], f64), 1.0)
            assert ((hi - lo) * n < 1.0).all(), "the uv box spans more than one texel"
            line = (np.ceil(lo * n - 0.5) + 0.5) / n
            out.append(np.where(line < hi, line, mid))
            cut |= line < hi
        return out, cut

    us, vs = (u - du, u + du), (v - dv, v + dv)
    (ucuts, ucut), (vcuts, vcut) = cuts(*us, 0), cuts(*vs, 1)
    k = np.ceil(llo)
    lcut = (k > llo) & (k < lhi)
    # the box's corners and centre for every pixel; the whole grid of piece corners for the pixels whose box is cut at all
    vals = [smp.sample(u, v, lam)] + [smp.sample(a, b, c) for a in us for b in vs for c in (llo, lhi)]
    lo, hi = np.min(vals, axis=0), np.max(vals, axis=0)
    s = ucut | vcut | lcut
    if s.any():
        more = [smp.sample(a[s], b[s], c[s]) for a in (*us, *ucuts) for b in (*vs, *vcuts) for c in (llo, lhi, np.where(lcut, k, llo))]
        lo[s], hi[s] = np.minimum(lo[s], np.min(more, axis=0)), np.maximum(hi[s], np.max(more, axis=0))
    return lo - SAMPLER_STEPS * U, hi + SAMPLER_STEPS * U


def byte_stats(got, lo, hi):
    """got [k, c] bytes against the value interval [lo, hi] [k, c]: bad (pixels with a byte outside the admissible ones), worst (the
    largest distance of a byte from the interval's middle as a share of the byte's half step plus the interval's half width: above 1
    is outside), undecided (share of pixels whose interval admits two bytes on some channel), off (share of pixels with a byte that is
    not the byte of the interval's middle: an admissible byte one step from it), width (the widest interval, in bytes)"""
    got = np.asarray(got, dtype=np.int64)
    blo, bhi = unorm8(lo), unorm8(hi)
    bad = ((got < blo) | (got > bhi)).any(axis=1)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    k = max(len(got), 1)
    return {"bad": int(bad.sum()), "worst": float((np.abs(got - 255.0 * mid) / (0.5 + 255.0 * half)).max()) if got.size else 0.0,
            "undecided": float((blo != bhi).any(axis=1).sum()) / k, "off": float((got != unorm8(mid)).any(axis=1).sum()) / k, "width": float((255.0 * (hi - lo)).max()) if got.size else 0.0,
            "pixels": len(got)}


def surface_stats(C, lo, hi):
    """the C plane's words [k] (roughness, metallic, AO = sample.x, all three from the same texture)"""
    C = np.asarray(C, dtype=np.int64)
    got = np.stack([C & 255, (C >> 8) & 255, (C >> 16) & 255], axis=1)
    e = ENCODE_STEPS * U
    return byte_stats(got, np.repeat(lo[:, :1], 3, axis=1) - e, np.repeat(hi[:, :1], 3, axis=1) + e)


def transcendental_band(c):
    """the relative band of exp2(2.2 log2 c) at c in [0, 1] (0 at c = 0: the result is exactly 0)"""
    with np.errstate(divide="ignore"):
        lg = np.abs(np.log2(np.where(c > 0, c, 1.0)))
    return np.where(c > 0, np.log(2.0) * 2.2 * lg * (2.0 ** -23 + 2.0 ** -24) + 2.0 ** -23, 0.0)


def albedo_stats(smp, A, lo, hi):
    """the A plane's words [k] (albedo = sample.rgb ** 2.2); trans: the largest multiple of the transcendental band a byte needs"""
    A = np.asarray(A, dtype=np.int64)
    got = np.stack([A & 255, (A >> 8) & 255, (A >> 16) & 255], axis=1)
    lo, hi = np.clip(lo, 0.0, 1.0), np.clip(hi, 0.0, 1.0)
    e = ENCODE_STEPS * U
    plo, phi = smp.gamma(lo) - e, smp.gamma(hi) + e
    tlo, thi = smp.gamma(lo) * transcendental_band(lo), smp.gamma(hi) * transcendental_band(hi)
    st = byte_stats(got, plo - tlo, phi + thi)
    # byte g is admitted by k bands when [g - 1/2, g + 1/2) meets 255 [plo - k tlo, phi + k thi]
    below, above = 255.0 * plo - (got + 0.5), (got - 0.5) - 255.0 * phi
    with np.errstate(divide="ignore", invalid="ignore"):
        need = np.maximum(np.where(below > 0, below / (255.0 * tlo), 0.0), np.where(above > 0, above / (255.0 * thi), 0.0))
    st["trans"] = float(need.max()) if need.size else 0.0
    return st


def normal_stats(B, lo, hi, n, dn, t, dt):
    """the B plane's words [k] (the normal map): n, dn, t, dt the interpolated normal and tangent with their bands"""
    ts, dts = lo + hi - 1.0, (hi - lo) + U
    return check_normal_bytes(np.asarray(B), *mapped_normal(n, dn, t, dt, ts=ts, dts=dts))
