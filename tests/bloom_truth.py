"""Float64 truth for the bloom pyramid: the prefilter (bloom_prefilter.hlsl:17-60), the separable nine-tap blur (blur.hlsli:24-89),
the upsample-add (bloom_upsample_add.hlsl:13-25), the merge (bloom_merge.hlsl:7-11) and BloomPass::Execute
(DeferredPipeline.cpp:400-570), restated in plain numpy on the exact half inputs, with the bands inside which an fp32 implementation
may differ from it, the case sets the CPU and GPU tests share, and the assertions both run.  No GPU and no oracle in here:
tests/test_bloom_truth_cpu.py holds the oracle to these assertions, tests/test_gpu_bloom_truth.py the kernels.

What is specification and what is truth.  Texture2D<half4>.SampleLevel(LinearClamp) is modelled as D3D states it: the scaled
coordinate u * size is clamped to [-1.5, size + 1.5] and snapped to x.8 fixed point (round to nearest), then the half-texel offset
is removed, the two indices are clamped, and a tap whose weight is exactly 0 does not contribute.  The COORDINATE is part of the
specification and is evaluated in float32 with the shader's own expressions: ((x + 0.5f) * tx) * size with tx = 1.0f / ow for the
blur, the 256-thread group's eight halo entries from max(uv - 4 tx, 0) / min(uv + 4 tx, 1) of the group's first and last four
threads (threads past the image edge of a partial last group included), x * tx + off * tx (no + 0.5) for the prefilter.  A float64
coordinate would define another filter: one fp32 ulp of u * size * 256 is 2^-24 * size * 256, i.e. 1/32 of a snap step at a level
width of 2048 and 1/8 at 8192, so at sizes that are no exact multiple the float32 product lands on the other side of a snap
boundary at some texels (513 -> 256 is in the case set for that), and the halo expression is not the neighbouring thread's
(test_halo_from_the_neighbouring_groups_coordinate_is_rejected).  Everything after the snap is float64: the tap weights (multiples
of 1/256), the lerps, the nine weights and the luminance coefficients as the float32 constants they are, the sums, the divisions.
tests/test_bloom_truth_cpu.py evaluates a blur stage and the prefilter in exact rationals and finds the float64 truth within 1e-13.

The bands are derived from the number formats, not tuned against either implementation.  u = 2^-24 is fp32's unit roundoff; k
roundings on top of each other cost gamma(k) = k u / (1 - k u) of the magnitude M = sum |weight * tap| they act on (Higham,
Accuracy and Stability of Numerical Algorithms, lemma 3.1).  A band has to hold for ANY fp32 evaluation of the stage's linear map,
because k_blur_up_poly (csrc/bloom.hip) is one that reorders it.

Blur stage, K_BLUR = 13 (band 13 u M).
* the bilinear sample: the texels are exact halves and 1 - f is exact (f is a multiple of 1/256).  A lerp is the product a (1 - f)
  (one rounding) and the fused b f + that (one rounding): 2 u of its magnitude; the y lerp stacks two more on the x lerps' results:
  K_SAMPLE = 4.  (Three fused lerps and their three 1 - f products; at an exact 2x size the products by 1/2, 1/4, 3/4 are exact and
  the sample costs less.  The band does not use that.)
* the nine multiply-accumulates v = fma(tap, w, v) round once each; the first term passes through nine of them, the last through
  one, and no association order of nine products nests deeper: K_GAUSS = 9 of sum |w tap|.  The weights are the float32 constants
  in truth and implementation alike and carry no error.
* the polyphase form of the 2x-up H stage needs less, K_POLY = 11 <= K_BLUR: its six coefficients E(j) are float64 sums of the nine
  DECIMAL weights rounded once to fp32 — the decimal 0.0148 and the constant 0.0148f differ by up to u, the rounding adds u: 2 u —,
  the six-tap filter rounds six times, the 1/4 | 3/4 row blend is a product and a fused add: 2; the same-size nine taps of the DUAL
  instance are exact texels through nine roundings (<= 11), and the pair sum rounds once more, which K_DUAL counts.
Upsample-add, K_DUAL = 14: each addend is a blur stage (13 u of its own M), the sum rounds once (u |T| <= u M); M is the two M's sum.
Merge, K_MERGE = 1: one fp32 add of two halves.  The float64 sum of two halves is exact (they span at most 51 bits); where that sum
is an fp32 number the add is exact as well and the band is ZERO, elsewhere u |T|.  This matters: sums of two halves of neighbouring
exponents land exactly on the midpoint between two halves one time in six on the noise frames, and a band of u |T| there would leave
16 % of the chain's texels undecided where the fp32 add leaves no freedom at all (2 % after the sharpening).
Prefilter: no single factor.  prefilter() propagates first-order absolute errors through the shader's expression, per sample:
  the sample 4 u of its magnitude per channel; brightness = max of three (1-Lipschitz: the largest of the three errors);
  threshold * knee one rounding; s0 = brightness - threshold + threshold * knee CANCELS: its error is ABSOLUTE, the operands' own
  plus 2 u (|brightness| + |threshold| + |threshold knee|) for two adds in either order, and stays that large while s0 goes through
  zero at the knee's lower edge; the clamp to [0, 2 threshold knee] is 1-Lipschitz (error 0 where s0 is below zero by more than its
  error, the cap's own 2 u threshold knee above the cap, and never more than the cap itself, so knee = 0 gives an exact 0); the
  divisor 4 threshold knee + 0.00001f two roundings, the IEEE divide one; brightness - threshold one rounding on top of the
  brightness' error, absolute again at the crossover; max(soft, brightness - threshold) takes the error of the larger branch, of
  both where their intervals overlap (the crossover); max(brightness, 0.00001f); the second divide; colour * contribution one
  rounding per channel; the luminance dot 4 u of sum |coefficient * channel| (three products, two sums, in any fusing); + 1 and the
  third divide one rounding each; colour * weight one.  The five-term sums round four times each.  The computed weights enter the
  numerator and the denominator of total / total_w alike, so a weight's error dw moves the mean by (colour_i - mean) dw / total_w,
  not by (|colour_i| + |mean|) dw / total_w; the sums' and the final divide's roundings are 5 u of |mean|.  The neglected products
  of two errors are covered by the factor 1 + 2^-10.  The result is 31 .. 38 u of |T| at the median of the noise frames (48 .. 51 u
  before the weights' correlation was used), 48 u at the 99th percentile and up to 114 u where a sample sits on the crossover at knee = 0 — wider than a crude
  16 u M, because the contribution's cancellation and the weight 1 / (luminance + 1) amplify the sample's 4 u three times over on
  the way to the mean; the undecided shares below are what it costs.
Alpha is the constant 1 the prefilter stores (band 0), and one constant per plane through every later stage, like the colours.

The assertions.  Per stage, for every texel and channel, alpha included: RN_half(T - B) <= got <= RN_half(T + B) (check_stage).  No
texel is left out; where the two ends differ ("undecided") the value must still be one of the two, and stage_conditions asserts on
the truth alone that the ends are never more than one half apart and that at most 2 % of a case's values are undecided.  End to end
(chain / check_chain, and up_level_interval for the fused up-level whose H result nobody sees): every stage after the prefilter is
monotone in its input (positive weights, clamp addressing, RN_half, the sums), x - K u |x| is increasing, and the prefilter's input
is exact, so the pyramid run once on RN_half(T - B) and once on RN_half(T + B) of every stage brackets every implementation that
meets the per-stage bands.  chain_conditions asserts that this interval is at most 2 halves wide at every texel and degenerate on
>= 95 % of them.  check_stage also returns the worst |v - T| / B that the stored halves prove (v: the real nearest T among those
that round to the stored half) — how much of the band an implementation visibly uses.

Measured (the undecided shares are the truth's own; noise / smooth / black / subnormal / bright where a shape has all five planes):
  blur_h  128x64->64x32 0.17 0.17 0 0.05 0.28 %   64x32 same size 0.13 0.12 0 0.01 0.24   32x16->64x32 0.22 0.23 0 0.10 0.18
          301x21->150x10 0.15   45x6->22x3 0   22x11->45x22 0.20   513x33->256x16 0.20   1200x6->600x3 0.11   1x40, 40x1 0
  blur_v  128x64->64x32 0.15 0.15 0 0.06 0.18 %   64x32 same size 0.15 0.15 0 0.06 0.24   32x16->64x32 0.20 0.21 0 0.10 0.21
          301x21->150x10 0.18   45x6->22x3 1.14 (3 of 264)   22x11->45x22 0.10   513x33->256x16 0.16   6x1200->3x600 0.28
          1x40 0.62 (1 of 160)   40x1 0
  up-level, noise: H 0.06 .. 0.24 %, V 0.11 .. 0.21 % over 32x16, 48x16, 5x20, 200x152 -> twice that, DUAL and not
  prefilter 128x64 (1, 0.5) 0.45 0.46 0 0 0.54 %   (0.25, 0.1) 0.37 0.35 0 0 0.42   (1, 0) 0.46 0.46 0 0 0.54   (0, 0.5) 0.43 0.43 0 0 0.71
            131x77 (1, 0.5) 0.50 0.51 0 0 0.54 %   (0.25, 0.1) 0.43 0.43 0 0 0.43   (1, 0) 0.46 0.47 0 0 0.54   (0, 0.5) 0.38 0.39 0 0.08 0.35
            2x2 0 throughout.  The subnormal plane of the prefilter cases holds multiples of 2^-22 (plane(step=4)): at threshold 0
            the contribution is exactly 1 and the mean of quarter-weighted multiples of 2^-24 sits ON the midpoints of the
            subnormal lattice (3.1 % undecided at 128x64) — an input replaced, not a cap raised.
  chain   interval width / degenerate share, noise and smooth: 256x128 2 / 98.45 % and 98.10 %   320x180 2 / 97.96 % and 98.11 %
          400x300 2 / 98.47 % and 98.42 %   16x16 1 / 99.80 % and 99.02 %   17x31 2 and 1 / 99.67 % and 99.05 %;
          black and subnormal frames: width 0, 100 % (a subnormal frame is below the threshold: the pyramid is zeros)
  worst visible |v - T| / B, the CPU oracle and the MI355X kernels alike (the staged kernels and k_blur_hv are bit-identical to
  the oracle on every case here): blur_h 0.10, blur_v 0.14, upsample_add 0.14, prefilter 0.04, merge 0 — the shader's order uses
  a seventh of the band at most.
  k_blur_up_poly on the MI355X (knobs build, forced on): of the values of an up-level 200x152 -> 400x304, 17 (DUAL) and 15 of
  486 400 differ from the oracle's two staged calls on the noise planes, 8 and 4 on the subnormal planes, 1 of 12 288 at 48x16, none
  at 32x16 and 5x20; all by one half, at texels where the propagated interval is one half wide: the kernel took one end, the oracle the other.  Whole
  pyramid with every up-level polyphase: 256x128 5 (noise) and 3 (smooth, one of them 2 halves) of 131 072 values differ, 96x32 0
  and 2 of 12 288, all inside the chain interval.  Product library, 1024x400 -> 2048x800 (400 tiles): 175 (DUAL) and 408 of
  6 553 600 values differ by one half, all inside.  k_blur_hv TH = 32 under the shader-order switch (960x480 -> 1920x960): none differ.
  So the "<= 1 fp16 ULP per stage, <= 2 end to end" allowance of tests/test_gpu_parity.py is sound: where the polyphase kernel and
  the oracle differ, both are admissible roundings of the same truth.
  The fused kernels' premise (tap1d's integer taps, the prefilter's quad means) holds at every size 1 .. 8192 they are launched for.

The tiled pass (pbr_bloom_tiled, the multi-GPU path).  tiled_chain is the same interval propagation started from a GIVEN level 1 of
the extended tile E and merged over merge_rect; no new band.  What the kernels add to that — the up-pass on rectangles, the kernel
chosen by the rectangle's tiles, the first tile, buf_origin — is restated as integers: up_pass_rects (the rule of csrc/bloom.hip),
up_pass_dependency (the exact rectangles from tap1d's taps), up_kernel / tiled_kernels (launch_hv's choice).  Proven on the CPU
(tests/test_bloom_truth_cpu.py): the rule's rectangles contain the exact ones with 1 .. 2 texels to spare per side at level 1 and
2 .. 3 at levels 2 .. 4, for every residue mod 32 of origin and size; an interior pixel depends on level-1 texels at most 192 pixels
outside an interior aligned to 16, 195 with the prefilter's reads (202 / 205 at any alignment), under the apron of 256; behind that
apron a rank's float64 values are the frame's own, bit for bit (and stay so down to an apron of 144 / 160 on the two noise frames
tried: the half stores in between swallow what the far taps contribute).
Measured on the MI355X (tests/test_gpu_bloom_tiled_truth.py): TILED_SMALL and TILED_BIG intervals at most 2 wide, 0.9 .. 1.6 %
undecided; every merged value inside, shrunk and whole up-pass alike.  2432 x 2672 (level 1: k_blur_hv/16 on the rectangle,
k_blur_up_poly on the whole level): 371 of 16 588 800 merged values differ between the two, by at most 2 half steps, all where the
interval is not degenerate; the other three big cases select the same kernels either way and are bit-identical.  The tail's histogram
equals pbr_lum_histogram on the merged window exactly; against the float64 bins of the stored output it differs by 0 .. 1 pixel on
the small cases and 10 .. 43 of 1.6 .. 8.3 M on the big ones, every one of them among the 2 .. 5 in ten thousand pixels that
exposure_truth calls ambiguous (within its derived band of a bin edge) and counted in the bin on the other side of that edge —
which is what check_tiled asserts: exact where the truth decides.
"""
import numpy as np

U = 2.0 ** -24
GAUSS32 = np.array([0.0148, 0.0459, 0.1050, 0.1941, 0.2803, 0.1941, 0.1050, 0.0459, 0.0148], dtype=np.float32)   # blur.hlsli:17
GAUSS = GAUSS32.astype(np.float64)
LUMA = np.array([0.2126, 0.7152, 0.0722], dtype=np.float32).astype(np.float64)                                      # global.hlsli:140-143
EPS = float(np.float32(0.00001))
THRESHOLD, KNEE = 1.0, 0.5
K_SAMPLE, K_GAUSS = 4, 9
K_BLUR = K_SAMPLE + K_GAUSS          # 13
K_DUAL = K_BLUR + 1                  # 14
K_MERGE = 1
K_POLY = 11                          # what the polyphase form needs at most (module docstring)
assert K_POLY <= K_BLUR
SECOND_ORDER = 1.0 + 2.0 ** -10      # prefilter: the first-order propagation's neglected products of two errors
UNDECIDED_CAP = 0.02
CHAIN_WIDTH_CAP = 2
CHAIN_DEGENERATE_MIN = 0.95
GROUP, HALO, CACHE = 256, 4, 264
F32 = np.float32


def gamma(k):
    """(1 + u)^k - 1 <= k u / (1 - k u): k roundings on top of each other"""
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------------------------ half helpers
def rn_half(x):
    """float64 -> the nearest half (ties to even, overflow to Inf), one rounding"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float16)


def half_key(x):
    """halves -> integers in value order (+0 and -0 both 0)"""
    b = np.ascontiguousarray(x, dtype=np.float16).view(np.uint16).astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


def half_width(lo, hi):
    """how many halves hi lies above lo"""
    return half_key(hi) - half_key(lo)


def _cell(h):
    """the reals that round to the finite half h: (lower, upper) midpoints to its neighbours, as float64"""
    h = np.ascontiguousarray(h, dtype=np.float16)
    v = h.astype(np.float64)
    with np.errstate(over="ignore"):
        dn = np.nextafter(h, np.float16(-np.inf)).astype(np.float64)
        up = np.nextafter(h, np.float16(np.inf)).astype(np.float64)
    dn = np.where(np.isfinite(dn), dn, -65536.0)       # the neighbours of +-65504 in an unbounded exponent range
    up = np.where(np.isfinite(up), up, 65536.0)
    return (v + dn) / 2, (v + up) / 2


# ------------------------------------------------------------------------------------------------------------------ the sampler
def sample_coord(u, size, wrap=False):
    """The sampler's addressing along one axis.  u: float32 array of normalized coordinates, as the shader computed them.
    Returns (i0, i1, f): the two CLAMPED texel indices and the second one's weight, a multiple of 1/256 (float64).  float32 up to the
    snap, like the coordinate: the product u * size, the clamp to [-1.5, size + 1.5], the snap floor(c * 256 + 0.5) / 256."""
    u = np.asarray(u, dtype=F32)
    assert u.dtype == F32
    c = u * F32(size)
    c = np.where(c == c, c, F32(0.5))
    c = np.minimum(np.maximum(c, F32(-1.5)), F32(size) + F32(1.5))
    x = np.floor(c * F32(256.0) + F32(0.5)) * F32(1.0 / 256.0) - F32(0.5)
    assert x.dtype == F32
    fl = np.floor(x)
    i0 = fl.astype(np.int64)
    f = (x - fl).astype(np.float64)
    if wrap:                                               # the defect tests' wrong addressing mode
        return i0 % size, (i0 + 1) % size, f
    return np.clip(i0, 0, size - 1), np.clip(i0 + 1, 0, size - 1), f


def lerp(a, b, f):
    """a (1 - f) + b f; a tap with weight exactly 0 does not contribute"""
    zero = f == 0.0
    if zero.all():
        return a
    with np.errstate(invalid="ignore", over="ignore"):
        r = a * (1.0 - f) + b * f
    return np.where(zero, a, r) if zero.any() else r


def cache_coords(out_size):
    """blur.hlsli:24-55 along the blurred axis: the float32 coordinate of every Cache[] entry of every 256-thread group,
    [groups, 264].  Entry t + 4 is thread t's own ((x + 0.5f) * tx); entries 0 .. 3 are max(uv - 4 tx, 0) of threads 0 .. 3 and
    entries 260 .. 263 min(uv + 4 tx, 1) of threads 252 .. 255.  Threads past the image edge are included."""
    tx = F32(1.0) / F32(out_size)
    groups = -(-out_size // GROUP)
    x = (np.arange(groups)[:, None] * GROUP + np.arange(GROUP)[None, :]).astype(F32)
    uv = (x + F32(0.5)) * tx
    out = np.empty((groups, CACHE), dtype=F32)
    out[:, HALO:HALO + GROUP] = uv
    out[:, :HALO] = np.maximum(uv[:, :HALO] - F32(4.0) * tx, F32(0.0))
    out[:, HALO + GROUP:] = np.minimum(uv[:, GROUP - HALO:] + F32(4.0) * tx, F32(1.0))
    return out


def plain_coords(out_size):
    """(x + 0.5f) * tx of every output texel along the axis that is not blurred"""
    return (np.arange(out_size).astype(F32) + F32(0.5)) * (F32(1.0) / F32(out_size))


# ------------------------------------------------------------------------------------------------------------------ the stages
def _with_abs(a):
    a = np.asarray(a).astype(np.float64)
    return a if (a >= 0).all() else np.concatenate([a, np.abs(a)], axis=-1)


def _split(t, channels):
    return (t, t) if t.shape[-1] == channels else (t[..., :channels], t[..., channels:])


def _blur_rows(img, ow, oh, weights=GAUSS, cache=None, wrap=False, swap=False):
    """the H pass on img [ih, iw, c] -> (T, M) [oh, ow, c]: bilinear samples at the cache coordinates, nine weighted taps.  weights,
    cache (other Cache[] coordinates), wrap and swap (the two taps' weights exchanged) exist for the defect tests."""
    ih, iw, ch = img.shape
    a = np.ascontiguousarray(_with_abs(img).transpose(0, 2, 1))      # [ih, c, iw]: the blurred axis last
    j0, j1, fy = sample_coord(plain_coords(oh), ih, wrap)
    rows = lerp(a[j0], a[j1], fy[:, None, None])
    cc = cache_coords(ow) if cache is None else cache
    i0, i1, fx = sample_coord(cc.reshape(-1), iw, wrap)
    if swap:
        i0, i1 = i1, i0
    s = lerp(rows[..., i0], rows[..., i1], fx[None, None, :])       # [oh, c, groups * 264]: every Cache[] entry
    taps = np.zeros((CACHE, GROUP))                                  # output t of a group taps Cache[t .. t + 8]
    for k in range(9):
        taps[np.arange(GROUP) + k, np.arange(GROUP)] = weights[k]
    groups = cc.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        if np.isfinite(s).all():
            out = (s.reshape(-1, CACHE) @ taps).reshape(oh, a.shape[1], groups * GROUP)[..., :ow]
        else:                                                        # 0 * Inf: keep the zeros of the tap matrix out of the sums
            s4 = s.reshape(oh, a.shape[1], groups, CACHE)
            out = np.zeros((oh, a.shape[1], groups, GROUP))
            for k in range(9):
                out += weights[k] * s4[..., k:k + GROUP]
            out = out.reshape(oh, a.shape[1], groups * GROUP)[..., :ow]
    return _split(np.ascontiguousarray(out.transpose(0, 2, 1)), ch)


def blur_h(img, ow, oh, **kw):
    """blur_horizontal (blur.hlsli:24-55): (T, M), the value in front of the half store and sum |weight * tap|"""
    return _blur_rows(np.asarray(img), ow, oh, **kw)


def blur_v(img, ow, oh, **kw):
    """blur_vertical (blur.hlsli:58-89)"""
    t, m = _blur_rows(np.asarray(img).transpose(1, 0, 2), oh, ow, **kw)
    return t.transpose(1, 0, 2), m.transpose(1, 0, 2)


def upsample_add(upper, lower):
    """bloom_upsample_add.hlsl:13-25: H(lower at upper's size) + H(upper)"""
    uh, uw = upper.shape[:2]
    tl, ml = blur_h(lower, uw, uh)
    tu, mu = blur_h(upper, uw, uh)
    return tl + tu, ml + mu


def merge(hdr, src):
    """bloom_merge.hlsl:7-11"""
    a, b = np.asarray(hdr).astype(np.float64), np.asarray(src).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = a + b                                                    # exact: two halves span at most 51 bits
        exact = ~np.isfinite(t) | (t.astype(F32).astype(np.float64) == t)
    return t, np.where(exact, 0.0, np.abs(t))


def band(k, m):
    return gamma(k) * m


def prefilter(img, threshold=THRESHOLD, knee=KNEE, half_texel=False, luma=LUMA):
    """bloom_prefilter.hlsl:17-60 -> (T, M) [h >> 1, w >> 1, 4] with band = U * M: M is the propagated error in units of u, the
    absolute terms of the cancellations included (module docstring).  half_texel and luma exist for the defect tests."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    ow, oh = w >> 1, h >> 1
    a, mag = img[..., :3].astype(np.float64), np.abs(img[..., :3].astype(np.float64))
    th, kn = float(F32(threshold)), float(F32(knee))
    tk = th * kn
    e_tk = U * abs(tk)
    tx, ty = F32(1.0) / F32(ow), F32(1.0) / F32(oh)
    ux = np.arange(ow).astype(F32) * tx
    vy = np.arange(oh).astype(F32) * ty
    if half_texel:
        ux, vy = (np.arange(ow).astype(F32) + F32(0.5)) * tx, (np.arange(oh).astype(F32) + F32(0.5)) * ty
    cols, e_cols, wgts, e_wgts = [], [], [], []
    g4 = gamma(K_SAMPLE)
    with np.errstate(all="ignore"):
        for ox, oy in ((0, 0), (-1, -1), (-1, 1), (1, -1), (1, 1)):
            i0, i1, fx = sample_coord(ux + F32(ox) * tx, w)
            j0, j1, fy = sample_coord(vy + F32(oy) * ty, h)

            def bil(p):
                r0, r1 = p[j0], p[j1]
                return lerp(lerp(r0[:, i0], r0[:, i1], fx[None, :, None]), lerp(r1[:, i0], r1[:, i1], fx[None, :, None]), fy[:, None, None])
            c, mc = bil(a), bil(mag)
            ec = g4 * mc
            br, e_br = c.max(-1), ec.max(-1)
            s0 = br - th + tk
            e_s0 = e_br + e_tk + 2 * U * (np.abs(br) + abs(th) + abs(tk))
            cap, e_cap = 2 * tk, 2 * e_tk
            s1 = np.clip(s0, 0.0, cap)
            e_s1 = np.where(s0 + e_s0 <= 0.0, 0.0, np.where(s0 - e_s0 >= cap + e_cap, e_cap, np.maximum(e_s0, e_cap)))
            e_s1 = np.minimum(e_s1, cap + e_cap)
            d = 4 * tk + EPS
            e_d = 4 * e_tk + U * d
            soft = s1 / d
            e_soft = e_s1 / d + soft * (e_d / d + U)
            lin = br - th
            e_lin = e_br + U * np.abs(lin)
            num = np.maximum(soft, lin)
            e_num = np.where(soft - e_soft > lin + e_lin, e_soft, np.where(lin - e_lin > soft + e_soft, e_lin, np.maximum(e_soft, e_lin)))
            den = np.maximum(br, EPS)
            e_den = np.where(br + e_br < EPS, 0.0, e_br)
            con = num / den
            e_con = e_num / den + np.abs(con) * (e_den / den + U)
            col = c * con[..., None]
            e_col = np.abs(c) * e_con[..., None] + np.abs(con)[..., None] * ec + U * np.abs(col)
            lum = col @ luma
            e_lum = e_col @ luma + 4 * U * (np.abs(col) @ luma)
            p = lum + 1.0
            e_p = e_lum + U * np.abs(p)
            wgt = 1.0 / p
            e_w = np.abs(wgt) * (e_p / np.abs(p) + U)
            cols.append(col); e_cols.append(e_col); wgts.append(wgt); e_wgts.append(e_w)
        tw = sum(wgts)[..., None]
        tot = sum(c * w[..., None] for c, w in zip(cols, wgts))
        out = tot / tw                                               # every weight is positive: the shader's `if (total_w > 0)` holds
        # the computed weights enter numerator and denominator alike: out~ = sum(col~ w~) / sum(w~), so a weight's error moves the
        # mean by (col_i - out) dw_i / tw, not by (|col_i| + |out|) dw_i / tw
        e_num = sum(w[..., None] * ec_ + U * np.abs(c * w[..., None]) for c, ec_, w in zip(cols, e_cols, wgts))
        e_num += 4 * U * sum(np.abs(c * w[..., None]) for c, w in zip(cols, wgts))
        e_wts = sum(np.abs(c - out) * ew[..., None] for c, ew in zip(cols, e_wgts))
        e_out = ((e_num + e_wts) / tw + np.abs(out) * (4 * U + U)) * SECOND_ORDER
    t = np.concatenate([out, np.ones((oh, ow, 1))], axis=-1)
    m = np.concatenate([e_out / U, np.zeros((oh, ow, 1))], axis=-1)
    return t, m


def up_level_h(upper, lower, ow, oh):
    """the H stage of one upsample level: (T, M, band factor) of H(lower at ow x oh) [+ H(upper)]"""
    if upper is None:
        return (*blur_h(lower, ow, oh), K_BLUR)
    return (*upsample_add(upper, lower), K_DUAL)


def up_level(upper, lower, ow, oh):
    """one upsample level as pbr_bloom_up_level states it: V(RN_half(H(upper) + H(lower at ow x oh))), upper may be None.  Returns
    ((T, M) of the H stage, (T, M) of the V stage on the rounded truth of the H stage, the H stage's band factor)."""
    th, mh, k = up_level_h(upper, lower, ow, oh)
    return (th, mh), blur_v(rn_half(th), ow, oh), k


def up_level_interval(upper, lower, ow, oh):
    """(lo, hi) of the level's output, whose H result nobody sees: the two stages' bands propagated like the chain's"""
    th, mh, k = up_level_h(upper, lower, ow, oh)
    lo_h, hi_h = stage_interval(th, band(k, mh))
    tl, ml = blur_v(lo_h, ow, oh)
    tu, mu = (tl, ml) if np.array_equal(lo_h.view(np.uint16), hi_h.view(np.uint16)) else blur_v(hi_h, ow, oh)
    return _shifted(tl, -band(K_BLUR, ml)), _shifted(tu, band(K_BLUR, mu))


# ------------------------------------------------------------------------------------------------------------------ the chain
class Ops:
    """the five stage functions of the chain on half arrays; side -1 / 0 / +1: RN_half(T - B) / RN_half(T) / RN_half(T + B)"""

    def __init__(self, side=0, threshold=THRESHOLD, knee=KNEE):
        self.side, self.threshold, self.knee = side, threshold, knee

    def _r(self, tm, k):
        t, m = tm
        return _shifted(t, self.side * band(k, m))

    def prefilter(self, img):
        t, m = prefilter(img, self.threshold, self.knee)
        return _shifted(t, self.side * U * m)

    def blur_h(self, src, ow, oh):
        return self._r(blur_h(src, ow, oh), K_BLUR)

    def blur_v(self, src, ow, oh):
        return self._r(blur_v(src, ow, oh), K_BLUR)

    def upsample_add(self, upper, lower):
        return self._r(upsample_add(upper, lower), K_DUAL)

    def merge(self, hdr, src):
        return self._r(merge(hdr, src), K_MERGE)


def run_chain(img, ops):
    """BloomPass::Execute (DeferredPipeline.cpp:400-570) from stage functions: levels (w >> l, h >> l), prefilter, three H + V
    down levels, three upsample-add + V levels, the merge level's H + V, the merge.  Returns the merged image."""
    h, w = img.shape[:2]
    a = {1: ops.prefilter(img)}
    for l in (1, 2, 3):
        ow, oh = w >> (l + 1), h >> (l + 1)
        a[l + 1] = ops.blur_v(ops.blur_h(a[l], ow, oh), ow, oh)
    for l in (3, 2, 1):
        a[l] = ops.blur_v(ops.upsample_add(a[l], a[l + 1]), w >> l, h >> l)
    return ops.merge(img, ops.blur_v(ops.blur_h(a[1], w, h), w, h))


def up_pass_from_level1(level1, ops, ew, eh, after_up=None):
    """run_chain between its prefilter and level 0: the three down levels and the three up levels of an ew x eh frame whose level 1
    [eh / 2, ew / 2, 4] is given.  Returns the finished level 1.  after_up(level, result) -> result exists for the defect tests."""
    a = {1: np.ascontiguousarray(level1, dtype=np.float16)}
    assert a[1].shape[:2] == (eh >> 1, ew >> 1)
    for l in (1, 2, 3):
        ow, oh = ew >> (l + 1), eh >> (l + 1)
        a[l + 1] = ops.blur_v(ops.blur_h(a[l], ow, oh), ow, oh)
    for l in (3, 2, 1):
        a[l] = ops.blur_v(ops.upsample_add(a[l], a[l + 1]), ew >> l, eh >> l)
        if after_up is not None:
            a[l] = after_up(l, a[l])
    return a[1]


def run_from_level1(level1, ops, ew, eh, after_up=None):
    """run_chain after its prefilter and before its merge: what the merge adds, [eh, ew, 4] half"""
    return ops.blur_v(ops.blur_h(up_pass_from_level1(level1, ops, ew, eh, after_up), ew, eh), ew, eh)


def level0_truth(level1):
    """the float64 truth T of what the merge adds, in front of its half store, every earlier stage being its rounded truth"""
    eh, ew = 2 * level1.shape[0], 2 * level1.shape[1]
    ops = Ops(0)
    return blur_v(ops.blur_h(up_pass_from_level1(level1, ops, ew, eh), ew, eh), ew, eh)[0]


def window(img, rect, origin=(0, 0)):
    """the texels of rect = (x, y, w, h) of an image whose texel [0, 0] sits at `origin`"""
    x, y, w, h = rect
    return img[y - origin[1]:y - origin[1] + h, x - origin[0]:x - origin[0] + w]


def tiled_chain(level1, hdr, hdr_rect, merge_rect, ops=None):
    """pbr_bloom_tiled (csrc/bloom.hip): BloomPass::Execute minus its prefilter on the extended tile E whose half level-1 plane
    [eh / 2, ew / 2, 4] is GIVEN, merged into the HDR texels of merge_rect = (x, y, w, h) of E.  hdr [h, w, 4] holds hdr_rect of E.
    Returns (lo, hi) over merge_rect: the chain's interval propagation, nothing new in it — the pyramid is that of E (clamped at
    E's edges, every level whole), the bands are K_BLUR, K_DUAL and K_MERGE.  That the kernels run the up-pass on rectangles only
    is their business: up_pass_dependency says which texels the merged rectangle reads.  With `ops` one run of those stage
    functions instead of the two ends."""
    level1 = np.ascontiguousarray(level1, dtype=np.float16)
    assert (level1.astype(np.float32) >= 0).all() and (np.asarray(hdr).astype(np.float32) >= 0).all()
    eh, ew = 2 * level1.shape[0], 2 * level1.shape[1]
    mine = window(np.asarray(hdr), merge_rect, hdr_rect[:2])
    assert mine.shape[:2] == (merge_rect[3], merge_rect[2]), "merge_rect outside hdr_rect"

    def run(o):
        return o.merge(mine, window(run_from_level1(level1, o, ew, eh), merge_rect))
    return run(ops) if ops is not None else (run(Ops(-1)), run(Ops(+1)))


def chain(img, threshold=THRESHOLD, knee=KNEE):
    """(lo, hi): the halves between which every implementation that meets the per-stage bands must land, per texel.  Every stage
    after the prefilter is monotone in its input (positive weights, clamp addressing, RN_half, the sums), the prefilter's input is
    exact; inputs must be non-negative for T - B and T + B to be monotone too."""
    assert (np.asarray(img).astype(np.float32) >= 0).all()
    return run_chain(img, Ops(-1, threshold, knee)), run_chain(img, Ops(+1, threshold, knee))


# ------------------------------------------------------------------------------------------------------------------ the assertions
def _shifted(t, b):
    """RN_half(t + b); an infinite t (a sum of halves that overflowed upstream) stays what it is"""
    with np.errstate(invalid="ignore"):
        return rn_half(np.where(np.isfinite(t), t + b, t))


def stage_interval(t, b):
    return _shifted(t, -b), _shifted(t, b)


def stage_conditions(t, b, what=""):
    """what the truth alone must meet before anything is compared with it: the undecided share under the cap and no interval wider
    than one half step.  Returns (lo, hi, undecided share)."""
    lo, hi = stage_interval(t, b)
    wd = half_width(lo, hi)
    und = float((wd != 0).mean())
    assert und <= UNDECIDED_CAP, f"{what}: {und:.4%} of the texels undecided, above the cap"
    assert wd.max() <= 1, f"{what}: an interval spans {int(wd.max())} half steps"
    return lo, hi, und


def visible_error(got, t, b):
    """per value: |v - T| / B for the real v nearest to T among those that round to the stored half — the smallest error the
    implementation can have made, in units of the band (0 where the band is 0 or the value is not finite)"""
    got = np.ascontiguousarray(got, dtype=np.float16)
    c0, c1 = _cell(got)
    with np.errstate(invalid="ignore", divide="ignore"):
        need = np.maximum(np.maximum(c0 - t, t - c1), 0.0)
        return np.where(np.isfinite(got.astype(np.float64)) & (b > 0), need / np.where(b > 0, b, 1.0), 0.0)


def check_stage(got, t, b, what=""):
    """RN_half(T - B) <= got <= RN_half(T + B) at every texel and channel.  Returns {"undecided", "worst"}: worst is the largest
    |v - T| / B that the stored halves prove, v being the nearest real that rounds to the stored half."""
    got = np.ascontiguousarray(got, dtype=np.float16)
    assert got.shape == t.shape, (what, got.shape, t.shape)
    lo, hi, und = stage_conditions(t, b, what)
    g = got.astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = (lo.astype(np.float64) <= g) & (g <= hi.astype(np.float64))
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} values outside the band; first at {i}: got {float(got[i])!r}, "
                             f"truth {t[i]!r} +- {b[i]:.3e} -> [{float(lo[i])!r}, {float(hi[i])!r}]")
    return {"undecided": und, "worst": float(visible_error(got, t, b).max())}


def chain_conditions(lo, hi, what=""):
    """the chain interval is at most 2 half steps wide everywhere and degenerate on >= 95 % of the texels: (max width, degenerate share)"""
    wd = half_width(lo, hi)
    assert wd.min() >= 0
    deg = float((wd == 0).mean())
    assert wd.max() <= CHAIN_WIDTH_CAP, f"{what}: the chain interval is {int(wd.max())} half steps wide"
    assert deg >= CHAIN_DEGENERATE_MIN, f"{what}: only {deg:.2%} of the chain interval degenerate"
    return int(wd.max()), deg


def check_chain(got, lo, hi, what=""):
    got = np.ascontiguousarray(got, dtype=np.float16)
    assert got.shape == lo.shape
    width, deg = chain_conditions(lo, hi, what)
    g = got.astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = (lo.astype(np.float64) <= g) & (g <= hi.astype(np.float64))
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} values outside the chain interval; first at {i}: got {float(got[i])!r}, "
                             f"interval [{float(lo[i])!r}, {float(hi[i])!r}]")
    return {"width": width, "degenerate": deg}


def output_histogram(image):
    """exposure_truth's 256 float64 counts of a stored image [h, w, 4]"""
    import exposure_truth as et
    return et.hist_of(et.image_bins(image)[0]).astype(np.int64)


def check_tiled(case, before, after, hist, lo, hi, what=""):
    """One pbr_bloom_tiled call under the truth.  before / after: the HDR buffer [rows of hdr_rect, hdr_pitch, 4] as uint16 bits;
    hist: the 256 counts the call added to zeros (None: a call without histogram); lo, hi: tiled_chain's interval.  The merged
    rectangle inside the interval at every texel and channel; every other texel of the buffer, the pitch padding included, keeps
    its bits; the histogram's sum is the rectangle's area and its counts are exposure_truth's bins of the stored output — exactly
    for every pixel that truth decides; a pixel within its band of a bin edge (two or three in ten thousand of these outputs) may
    be counted on either side (exposure_truth.check_histogram_of_output).  Returns check_chain's figures and those two counts."""
    (hx, hy, hw, hh), (mx, my, mw, mh) = case.hdr_rect, case.merge_rect
    assert before.shape == after.shape == (hh, case.hdr_pitch, 4) and before.dtype == after.dtype == np.uint16
    rows, cols = slice(my - hy, my - hy + mh), slice(mx - hx, mx - hx + mw)
    got = np.ascontiguousarray(after[rows, cols]).view(np.float16)
    r = check_chain(got, lo, hi, what)
    kept = after == before
    kept[rows, cols] = True
    assert kept.all(), f"{what}: {int((~kept).sum())} values outside the merged rectangle changed; first at {tuple(np.argwhere(~kept)[0])}"
    if hist is not None:
        h = np.asarray(hist).astype(np.int64).reshape(-1) & 0xFFFFFFFF
        assert int(h.sum()) == mw * mh, f"{what}: the histogram counts {int(h.sum())} pixels, the merged rectangle has {mw * mh}"
        import exposure_truth as et
        r["ambiguous"], r["other side"] = et.check_histogram_of_output(h, got)
    return r


# ------------------------------------------------------------------------------------------------------------------ the polyphase form
def poly_coefficients():
    """k_blur_up_poly's six coefficients E(-3 .. 2), recomputed: float64 sums of the nine decimal weights, rounded once to fp32"""
    g = {k - 4: v for k, v in enumerate([0.0148, 0.0459, 0.1050, 0.1941, 0.2803, 0.1941, 0.1050, 0.0459, 0.0148])}
    w = lambda k: g.get(k, 0.0)   # noqa: E731
    return np.array([F32(0.75 * w(2 * j) + 0.25 * w(2 * j + 2) + 0.75 * w(2 * j + 1) + 0.25 * w(2 * j - 1)) for j in range(-3, 3)], dtype=F32)


def poly_up_h(lower, upper=None):
    """The H stage of a 2x-up level in k_blur_up_poly's form, fp32 throughout: two six-tap filters on every coarse row with clamped
    taps (even output 2p: c[p-3 .. p+2] with E(-3 .. 2); odd output 2p + 1: c[p-2 .. p+3] with E(2 .. -3)), the 1/4 | 3/4 blend of
    neighbouring filtered rows (clamped), and with `upper` the nine same-size taps added.  Returns the fp32 value in front of the store."""
    lo = np.asarray(lower).astype(F32)
    lh, lw = lo.shape[:2]
    pe = poly_coefficients()
    p = np.arange(lw)
    ce = np.zeros_like(lo); co = np.zeros_like(lo)
    for j in range(6):
        ce = lo[:, np.clip(p - 3 + j, 0, lw - 1)] * pe[j] + ce
        co = lo[:, np.clip(p - 2 + j, 0, lw - 1)] * pe[5 - j] + co
    filt = np.empty((lh, 2 * lw, lo.shape[2]), dtype=F32)
    filt[:, 0::2], filt[:, 1::2] = ce, co
    y = np.arange(2 * lh)
    a = (y >> 1) - 1 + (y & 1)
    fy = np.where(y & 1, F32(0.25), F32(0.75)).astype(F32)[:, None, None]
    r0, r1 = filt[np.clip(a, 0, lh - 1)], filt[np.clip(a + 1, 0, lh - 1)]
    out = r1 * fy + r0 * (F32(1.0) - fy)
    if upper is not None:
        up = np.asarray(upper).astype(F32)
        x = np.arange(2 * lw)
        acc = np.zeros_like(up)
        for k in range(9):
            acc = up[:, np.clip(x - 4 + k, 0, 2 * lw - 1)] * GAUSS32[k] + acc
        out = out + acc
    assert out.dtype == F32
    return out


# ------------------------------------------------------------------------------------------------------------------ tap1d
M_SAME, M_DOWN, M_UP = 0, 1, 2


def tap1d(mode, p, in_size):
    """csrc/bloom.hip tap1d: the fused kernels' integer taps of output position p (any integer)"""
    p = np.asarray(p, dtype=np.int64)
    if mode == M_SAME:
        a, f = p, np.zeros(p.shape)
    elif mode == M_DOWN:
        a, f = 2 * p, np.full(p.shape, 0.5)
    else:
        a, f = (p >> 1) - 1 + (p & 1), np.where(p & 1, 0.25, 0.75)
    return np.clip(a, 0, in_size - 1), np.clip(a + 1, 0, in_size - 1), f


def canonical_taps(i0, i1, f):
    """two samples are the same function of the texels when these agree: a zero weight drops the second tap, and equal indices make
    the weight irrelevant (f and 1 - f are multiples of 1/256, so the lerp of a half with itself is exact in fp32)"""
    one = (f == 0.0) | (i0 == i1)
    return i0, np.where(one, i0, i1), np.where(one, 0.0, f)


# ------------------------------------------------------------------------------------------------------------------ the tiled schedule
MIPS = 5                             # PBR_BLOOM_MIPS: levels 0 .. 4


def _cdiv(a, b):
    """C's integer division: towards zero"""
    return -((-a) // b) if a < 0 else a // b


def up_pass_rects(merge_rect, ew, eh):
    """csrc/bloom.hip up_pass_rects, restated with C's truncating division: {level: (x, y, w, h)} for levels 1 .. 4, the rectangles
    the up-pass of a tiled frame is run on (levels 1 .. 3 have an up-pass; level 4's entry is computed and not used)"""
    x0, y0, x1, y1 = merge_rect[0], merge_rect[1], merge_rect[0] + merge_rect[2], merge_rect[1] + merge_rect[3]
    need = {}
    for l in range(1, MIPS):
        lw, lh = ew >> l, eh >> l
        x0, y0, x1, y1 = _cdiv(x0 - 4, 2) - 2, _cdiv(y0 - 4, 2) - 2, _cdiv(x1 + 4 + 1, 2) + 2, _cdiv(y1 + 4 + 1, 2) + 2
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, lw), min(y1, lh)
        need[l] = (x0, y0, x1 - x0, y1 - y0)
    return need


def _reads(mode, lo, hi, in_size):
    """[first, last + 1) of the input texels that the outputs lo .. hi - 1 of a nine-tap pass read along one axis: positions
    lo - 4 .. hi + 3 (any integer: tap1d clamps the texel, as the sampler does), a tap of weight 0 or a repeated index left out"""
    i0, i1, _ = canonical_taps(*tap1d(mode, np.arange(lo - 4, hi + 4), in_size))
    return int(min(i0.min(), i1.min())), int(max(i0.max(), i1.max())) + 1


def axis_dependency(lo, hi, size):
    """up_pass_dependency along one axis: merged texels lo .. hi - 1 of a level 0 of `size` texels -> ({level: range of the
    up-pass output read}, {level: range of the down-pass result read}), ranges [first, last + 1)"""
    up, down = {}, {}
    up[1] = _reads(M_UP, lo, hi, size >> 1)                        # level 0's H + V reads level 1's up-pass result
    for l in (1, 2, 3):                                            # up-level l: nine same-size taps on A l, nine 2x-up taps on the level below
        down[l] = _reads(M_SAME, *up[l], size >> l)
        below = _reads(M_UP, *up[l], size >> (l + 1))
        if l < 3:
            up[l + 1] = below
        else:
            down[4] = below                                        # level 4 has no up-pass: its down-pass result is read
    for l in (3, 2, 1):                                            # the down-pass of level l + 1 reads A l
        r = _reads(M_DOWN, *down[l + 1], size >> l)
        down[l] = (min(down[l][0], r[0]), max(down[l][1], r[1]))
    return up, down


def up_pass_dependency(merge_rect, ew, eh):
    """The exact rectangles, from tap1d's integer taps with clamping: ({level 1 .. 3: (x, y, w, h) of the up-pass output that the
    merged rectangle reads, directly or through the levels above}, {level 1 .. 4: the down-pass result read, by the up-pass and by
    the down-pass of the levels below}).  H and V are separable, so a rectangle is the product of the two axes' ranges."""
    ux, dx = axis_dependency(merge_rect[0], merge_rect[0] + merge_rect[2], ew)
    uy, dy = axis_dependency(merge_rect[1], merge_rect[1] + merge_rect[3], eh)
    box = lambda a, b: (a[0], b[0], a[1] - a[0], b[1] - b[0])   # noqa: E731
    return {l: box(ux[l], uy[l]) for l in ux}, {l: box(dx[l], dy[l]) for l in dx}


PREFILTER_READS = (-3, 2)            # half-res texel x reads the full-res pixels 2x - 3 .. 2x + 2 (five taps of 2 x 2 quads)


def tile_grid(rect, tw, th):
    """csrc/bloom.hip tile_grid: the tw x th tiles of a level that intersect rect -> (first tile (tx0, ty0), number of tiles)"""
    x, y, w, h = rect
    tx0, ty0 = x // tw, y // th
    return (tx0, ty0), (-(-(x + w) // tw) - tx0) * (-(-(y + h) // th) - ty0)


def up_kernel(rect, shader_order=False):
    """launch_hv's choice for a 2x-up level run on rect = (x, y, w, h) (a whole level: (0, 0, w, h)): the launch-log label, the
    first tile and the number of tiles.  128 x 32 tiles >= 400 and the shader-order switch off: k_blur_up_poly; else 64 x 32 tiles
    >= 900: k_blur_hv/32; else k_blur_hv/16 (64 x 16 tiles)."""
    first, n = tile_grid(rect, 128, 32)
    if n >= 400 and not shader_order:
        return "k_blur_up_poly", first, n
    first, n = tile_grid(rect, 64, 32)
    if n >= 900:
        return "k_blur_hv/32", first, n
    return ("k_blur_hv/16", *tile_grid(rect, 64, 16))


def tiled_kernels(merge_rect, ew, eh, shader_order=False, shrink=True):
    """[(level, label, first tile, tiles)] of the four 2x-up launches of pbr_bloom_tiled, levels 3, 2, 1, 0 in launch order; shrink
    False: the up-pass on whole levels (the knobs build's PBR_BLOOM_SHRINK=0)"""
    need = up_pass_rects(merge_rect, ew, eh)
    rects = {l: need[l] if shrink else (0, 0, ew >> l, eh >> l) for l in (3, 2, 1)}
    rects[0] = tuple(merge_rect)
    return [(l, *up_kernel(rects[l], shader_order)) for l in (3, 2, 1, 0)]


# ------------------------------------------------------------------------------------------------------------------ case sets
def _synth():
    from direct12pbrrenderer_amd import synth
    return synth


def plane(kind, w, h, seed=0, step=1):
    """an input plane [h, w, 4] half with constant alpha: noise (with impulses), smooth (noise without), black, subnormal (the half
    subnormals 2^-24 .. 2^-14), bright (near 60 000: the merge of two such planes overflows)"""
    if kind in ("noise", "smooth"):
        img = _synth().hdr_noise_image(w, h, seed=0xB100 + 977 * seed + w + 31 * h, impulse=kind == "noise")
    elif kind == "black":
        img = np.zeros((h, w, 4), dtype=np.float16)
    elif kind == "subnormal":
        rng = np.random.default_rng(0x5B + seed)
        img = (step * rng.integers(1, 0x0400 // step + 1, (h, w, 4))).astype(np.uint16).view(np.float16)   # patterns 1 .. 0x400: 2^-24 .. 2^-14
    elif kind == "bright":
        rng = np.random.default_rng(0xB16 + seed)
        img = (60000.0 - 2000.0 * rng.random((h, w, 4))).astype(np.float16)
    else:
        raise ValueError(kind)
    img = np.ascontiguousarray(img, dtype=np.float16)
    img[..., 3] = np.float16({"black": 0.0, "subnormal": 2.0 ** -20, "bright": 60000.0}.get(kind, 1.0))
    return img


KINDS = ("noise", "smooth", "black", "subnormal", "bright")
# (iw, ih, ow, oh)
BLUR_SHAPES = [(128, 64, 64, 32), (64, 32, 64, 32), (32, 16, 64, 32), (301, 21, 150, 10), (45, 6, 22, 3), (22, 11, 45, 22),
               (513, 33, 256, 16)]
BLUR_H_SHAPES = BLUR_SHAPES + [(1200, 6, 600, 3), (1, 40, 1, 40), (40, 1, 40, 1), (1, 40, 3, 80)]
BLUR_V_SHAPES = BLUR_SHAPES + [(6, 1200, 3, 600), (1, 40, 1, 40), (40, 1, 40, 1), (40, 1, 80, 3)]
PREFILTER_SHAPES = [(128, 64), (131, 77), (2, 2)]
PREFILTER_PARAMS = [(1.0, 0.5), (0.25, 0.1), (1.0, 0.0), (0.0, 0.5)]
CHAIN_SHAPES = [(256, 128), (320, 180), (400, 300), (16, 16), (17, 31)]
# (lw, lh) -> (2 lw, 2 lh)
UP_SHAPES = [(32, 16), (48, 16), (5, 20), (200, 152)]


def kinds_for(shape_index):
    """every shape sees noise; the first three also the smooth, black, subnormal and bright planes"""
    return KINDS if shape_index < 3 else ("noise",)


class Tiled:
    """one pbr_bloom_tiled call: the extended tile, the HDR buffer's rectangle and pitch, the merged rectangle, with or without the
    histogram, the kind of its two input planes"""

    def __init__(self, ew, eh, hdr_rect, hdr_pitch, merge_rect, kind, hist=True, shader_order=False):
        self.ew, self.eh, self.hdr_rect, self.hdr_pitch, self.merge_rect = ew, eh, tuple(hdr_rect), hdr_pitch, tuple(merge_rect)
        self.kind, self.hist, self.shader_order = kind, hist, shader_order
        assert ew % 16 == 0 and eh % 16 == 0 and hdr_pitch >= hdr_rect[2]

    @property
    def id(self):
        return f"{self.ew}x{self.eh}-{'_'.join(str(v) for v in self.merge_rect)}-{self.kind}" + ("-shader_order" if self.shader_order else "") + ("" if self.hist else "-nohist")

    def inputs(self):
        """(level 1 of E, the HDR texels of hdr_rect): non-negative planes with constant alpha, as chain requires, scaled by powers
        of two so that the merged luminance spreads over the histogram's bins instead of sitting in its last one (the planes reach
        8, with impulses 400, and the range ends at 4): level 1 by 2^-6 — the pyramid then adds 0.06 .. 0.5 —, the HDR rows by
        2^-1 .. 2^-10 in ten bands, so the rectangle has rows that the HDR texel dominates and rows that the pyramid does"""
        level1, hdr = plane(self.kind, self.ew >> 1, self.eh >> 1, seed=21), plane(self.kind, self.hdr_rect[2], self.hdr_rect[3], seed=22)
        rows = hdr.shape[0]
        level1[..., :3] = (level1[..., :3].astype(np.float32) * F32(2.0 ** -6)).astype(np.float16)
        hdr[..., :3] = (hdr[..., :3].astype(np.float32) * np.exp2(-(1.0 + np.arange(rows) * 10 // rows)).astype(F32)[:, None, None]).astype(np.float16)
        return level1, hdr

    def truth(self):
        return tiled_chain(*self.inputs(), self.hdr_rect, self.merge_rect)


# E 128 .. 400 on a side; merge rectangles at even origins that are multiples of no tile size (16, 32, 64, 128) unless they touch
# E's corner; hdr_rect larger than merge_rect and hdr_pitch larger than its width (odd ones too).  In order: a plain interior; the
# bottom-right corner of E; 8 x 8; no histogram; the top-left corner; a tall E and an odd-sized rectangle; a wide rectangle one
# texel inside hdr_rect's left edge; a level 4 of odd size (16 * 23 = 368 -> 23) and a narrow rectangle
TILED_SMALL = [
    Tiled(256, 128, (20, 10, 200, 100), 203, (34, 18, 150, 70), "noise"),
    Tiled(400, 304, (0, 0, 400, 304), 402, (2, 6, 398, 298), "smooth"),
    Tiled(128, 128, (50, 60, 30, 40), 37, (66, 70, 8, 8), "noise"),
    Tiled(320, 176, (6, 2, 300, 170), 301, (38, 22, 222, 100), "smooth", hist=False),
    Tiled(400, 128, (0, 0, 260, 90), 264, (0, 0, 130, 74), "noise"),
    Tiled(144, 400, (10, 100, 120, 250), 128, (42, 134, 71, 183), "smooth"),
    Tiled(272, 208, (16, 16, 240, 176), 250, (18, 50, 236, 100), "noise"),
    Tiled(368, 384, (128, 64, 130, 258), 131, (130, 66, 126, 254), "smooth"),
]
# the benchmark's rank shapes (the strong-scaling tile of 7680 x 4320 on 2 x 4, the weak-scaling rank in the bottom row, a wide low
# tile), as halo mode calls them: hdr_rect = the interior + 4 shaded pixels.  The kernels tiled_kernels gives them:
#   2432 x 2672: level 1 k_blur_hv/16 on the rectangle and k_blur_up_poly on the whole level; level 0 poly, first tile (2, 8)
#   3232 x 3312: level 1 poly, first tile (0, 3); level 0 poly, 2112 tiles, first tile (2, 8); under the shader-order switch
#                level 1 k_blur_hv/32 (23 x 49 tiles) and level 0 k_blur_hv/32
#   2816 x 896:  level 1 k_blur_hv/16, first tile (1, 3); level 0 poly, 441 tiles, first tile (1, 3)
TILED_BIG = [
    Tiled(2432, 2672, (252, 252, 1928, 2168), 1936, (256, 256, 1920, 2160), "noise"),
    Tiled(3232, 3312, (252, 252, 2728, 3060), 2730, (256, 256, 2720, 3056), "smooth"),
    Tiled(2816, 896, (132, 108, 2568, 648), 2570, (136, 112, 2560, 640), "noise"),
    Tiled(3232, 3312, (252, 252, 2728, 3060), 2730, (256, 256, 2720, 3056), "smooth", shader_order=True),
]
