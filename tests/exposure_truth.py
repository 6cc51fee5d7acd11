"""Float64 truth for the exposure stage: the luminance histogram (hdr_luminance_histogram.hlsl:23-59), the histogram average
(hdr_average_histogram.hlsl:26-73) and the ACES tone-map (hdr_tone_mapping.hlsl:9-52), restated in plain numpy on the exact half
values, with the bands inside which an fp32 implementation may differ from it, the case sets the CPU and GPU tests share, and the
assertions both run.  No GPU and no oracle in here: tests/test_exposure_truth_cpu.py holds the oracle to these assertions,
tests/test_gpu_exposure_truth.py the kernels.

The bands are derived from the number formats, not tuned.  u = 2^-24 is fp32's unit roundoff (one rounding is a relative error <= u,
one ULP is 2u).  The hardware transcendentals v_rcp_f32, v_log_f32 and v_exp_f32 are specified to 1 ULP in AMD's CDNA ISA guides
("Instruction Set Architecture: CDNA3 / CDNA4", VOP1 opcode tables), OCML's log2f / exp2f / expf to 1 ULP in the ROCm device-libs
documentation (OCML accuracy table), and the CPU oracle's libm is at least that good.

DELTA_H (histogram, in bins).  The kernels and the oracle compute, in fp32,
    lum = (r*0.2126f + g*0.7152f) + b*0.0722f;   w = ((log2(lum) - min_log) * inv_range) * 254 + 1
* lum: each weight is the decimal constant rounded to fp32 (u), each product rounds (u), two sums round (u each): for channels of one
  sign the relative error is <= 4u, in log2 units 4u / ln 2 = 3.4e-7.  (Mixed signs cancel: the mask widens by sum|terms| / |lum|.)
* log2: 1 ULP of a value below 32 in magnitude (1e-6 <= lum <= 65504: -19.94 .. 16), i.e. 2^-19 = 1.9e-6.
* - min_log: one rounding of a value below 32 in magnitude (|min_log| <= 12 here): 2^-20 = 9.5e-7.
  Sum 3.2e-6 in log2 units, times 254 / log_range bins per log2 unit (21.2 at range 12, 31.8 at range 8).
* * inv_range (itself a rounded 1 / range: u, and the product: u) on t in [0, 1], times 254: 508u; the product t * 254 < 256 rounds
  to 2^-17 = 128u, and so does the + 1.  Together 764u = 4.6e-5 bins.
delta_h_bound() evaluates this: 1.13e-4 bins at (-10, 12), 1.47e-4 at (-6, 8).  DELTA_H = 2^-12 = 2.44e-4 is the next power of two
above both.  Only the edges w = 2 .. 255 matter: below 1 and above 255 the value is clamped to exactly 1 or 255.  The `lum < 1e-6`
branch is ambiguous where lum is within its own error (4u sum|terms|) plus the rounding of the constant 1e-6f (u) of 1e-6.

DELTA_T (tone-map, in LSB of the 8-bit channel).  v = sat(pow(sat(ACES(x)), 0.454545)) * 255 + 0.5, x = c / (9.6 avg + 0.001).
* x: 9.6f (u), its product (u), 0.001f (< u of the sum), the sum (u), the division (u), c * inv_den (u): <= 6u.
* ACES numerator x (2.51 x + 0.03) and denominator x (2.43 x + 0.59) + 0.14: each constant u, each operation u, x's own 6u entering
  twice.  For x >= 0 all terms are positive and each is good to about 14u; for x < 0 the numerator's inner sum cancels at
  x = -0.03 / 2.51 = -0.01195 and its ABSOLUTE error stays 0.03 * 9u while its value goes through zero.  The denominator has no real
  root (its minimum is 0.104).  v_rcp_f32 2u, the product u.  tonemap_band() carries these per input as an interval [m_lo, m_hi].
* gc = exp2(0.454545f * log2(m)): log2 1 ULP of lg = 2u |lg|; the constant u and the product u; exp2's argument error e turns into
  the relative error e ln 2, and exp2 itself adds 2u: gc * (1.26 |lg| + 2) u.  gc |lg| <= 1.17 (at lg = -3.17), gc <= 1.
* gc * 255 (< 256: 128u) and + 0.5 (128u).
tonemap_band() evaluates v at both ends of the m interval and adds the rest.  Its maximum over every (half value, luminance) pair of
the case sets is 7.5e-4 LSB, met beside the numerator's zero crossing, and 2.9e-4 for non-negative inputs;
tests/test_exposure_truth_cpu.py asserts it stays below DELTA_T = 2^-10 = 9.8e-4, the next power of two above.

The average's bands.
* average bin = sum_i float(uint32(count_i * i)) / float(uint32(pixel_count - count_0)): the conversions round non-negative terms
  (u on the sum), the 8-level tree adds 8 roundings, the denominator's conversion and the division one each: AVG_BIN_REL = 11u
  = 6.6e-7 relative (1.4 * 2^-21).  Where every one of those operations is exact in fp32 (a one-bin frame of 3840 x 2160, say) the
  band is zero and the truncation is decided.
* lum = exp2(((bin - 1) / 254) * range + min_log): the exponent's division and product 2u of a value <= 12, its sum 2^-21 (magnitude
  below 16), times ln 2, plus exp2's 2u: LUM_REL = 1.45e-6.  Adjacent bins differ by 3.3 %, so with dt = 1e9 the result names its bin.
* result = prev + tt (lum - prev), tt = sat(1 - expf(-dt * 1.6f)): blend_bound() adds expf's 1 ULP and the argument's 2u (in tt), the
  difference's, the product's and the sum's roundings and LUM_REL: about 1e-6 of the result at dt = 1/60, prev = 0.18.
"""
import numpy as np

U = 2.0 ** -24
MIN_LOG = -10.0
LOG_RANGE = 12.0
EPSILON = 1e-6
DELTA_H = 2.0 ** -12
DELTA_T = 2.0 ** -10
AVG_BIN_REL = 11 * U
LUM_REL = 1.45e-6
HIST_CAP = 0.001      # share of a histogram case set that may be replaced as ambiguous
TONEMAP_CAP = 0.005   # share of the tone-map (value, luminance) cases that may be left out
AVERAGE_CAP = 0.01
TONEMAP_LUMS = (1e-4, 0.01, 0.18, 1.0, 50.0, 6000.0)


def delta_h_bound(min_log=MIN_LOG, log_range=LOG_RANGE):
    """the derived histogram band in bins (module docstring) for channels of one sign"""
    assert abs(min_log) <= 12.0                        # |log2 lum| < 20 and |log2 lum - min_log| < 32: ULP 2^-19, rounding 2^-20
    e_log = 4 * U / np.log(2.0) + 2.0 ** -19 + 2.0 ** -20
    return 254.0 / log_range * e_log + (508 + 128 + 128) * U


assert delta_h_bound() < DELTA_H and delta_h_bound(-6.0, 8.0) < DELTA_H


# ---------------------------------------------------------------------------------------------------------------- histogram
def bin_truth(r, g, b, min_log=MIN_LOG, log_range=LOG_RANGE):
    """(bin, ambiguous, edge_distance) per pixel.  edge_distance: how far the unfloored bin value is from the nearest edge 2 .. 255
    (inf where no edge is near: black, NaN, Inf, clamped)."""
    r, g, b = (np.asarray(c).astype(np.float64) for c in (r, g, b))
    with np.errstate(all="ignore"):
        tr, tg, tb = 0.2126 * r, 0.7152 * g, 0.0722 * b
        lum = tr + tg + tb
        mag = np.abs(tr) + np.abs(tg) + np.abs(tb)
        dark = lum < EPSILON                                       # NaN: false, takes the log branch like the shader's
        t = (np.log2(np.where(dark, 1.0, lum)) - min_log) / log_range
        w = t * 254.0 + 1.0                                        # unclamped, unfloored
        s = np.where(np.isnan(t), 0.0, np.clip(t, 0.0, 1.0))       # saturate(NaN) = 0
        bins = np.where(dark, 0.0, np.floor(s * 254.0 + 1.0)).astype(np.int64)
        k = np.clip(np.rint(w), 2.0, 255.0)                        # the nearest edge; w < 1 and w > 255 are clamped to exact values
        dist = np.where(dark | ~np.isfinite(w), np.inf, np.abs(w - k))
        cancel = np.where(np.isfinite(lum) & (lum != 0.0), mag / np.abs(lum), 1.0)
        amb = dist <= DELTA_H * np.maximum(cancel, 1.0)
        amb |= np.isfinite(lum) & (np.abs(lum - EPSILON) <= 4 * U * mag + U * EPSILON)
    return bins, amb, dist


def image_bins(image, min_log=MIN_LOG, log_range=LOG_RANGE):
    return bin_truth(image[..., 0], image[..., 1], image[..., 2], min_log, log_range)


def hist_of(bins):
    return np.bincount(np.asarray(bins).reshape(-1), minlength=256).astype(np.uint32)


def settle(image, min_log=MIN_LOG, log_range=LOG_RANGE):
    """(image with its ambiguous pixels replaced by black, how many, the closest approach to an edge among the pixels kept).  Asserts
    the cap on what may be replaced."""
    bins, amb, dist = image_bins(image, min_log, log_range)
    out = image.copy()
    out[amb, :3] = 0
    n = int(amb.sum())
    assert n <= HIST_CAP * amb.size, f"{n} of {amb.size} inputs are ambiguous: above the cap"
    return out, n, float(dist[~amb].min())


def check_histogram(got_hist, image, min_log=MIN_LOG, log_range=LOG_RANGE, times=1):
    """got_hist == the float64 counts of `image` ([h, w, 4], no ambiguous pixel in it), bin for bin"""
    bins, amb, _ = image_bins(image, min_log, log_range)
    assert not amb.any(), "the case builder left an ambiguous pixel in"
    want = hist_of(bins).astype(np.int64) * times
    got = np.asarray(got_hist).astype(np.int64).reshape(-1) & 0xFFFFFFFF
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"bins {bad[:8].tolist()}: got {got[bad[:8]].tolist()}, want {want[bad[:8]].tolist()} ({bad.size} bins differ)"


def bin_choices(image, min_log=MIN_LOG, log_range=LOG_RANGE):
    """(lowest, highest) bin per pixel in which a histogram inside the derived band may count it: equal wherever the truth decides,
    the two bins on either side of the edge for a pixel bin_truth calls ambiguous (0 and 1 for one at the dark threshold)"""
    bins, amb, _ = image_bins(image, min_log, log_range)
    r, g, b = (np.asarray(image[..., c]).astype(np.float64) for c in range(3))
    with np.errstate(all="ignore"):
        lum = 0.2126 * r + 0.7152 * g + 0.0722 * b
        k = np.clip(np.rint((np.log2(np.where(lum < EPSILON, 1.0, lum)) - min_log) / log_range * 254.0 + 1.0), 2.0, 255.0)
    k = np.where(np.isfinite(k), k, 2.0).astype(np.int64)
    edge = amb & ((bins == k) | (bins == k - 1))
    dark = amb & ~edge                                               # at the dark threshold: below it bin 0, above it bin 1
    assert (bins[dark] <= 1).all()
    return np.where(edge, k - 1, np.where(dark, 0, bins)), np.where(edge, k, np.where(dark, 1, bins))


def check_histogram_of_output(got_hist, image, min_log=MIN_LOG, log_range=LOG_RANGE):
    """got_hist against the float64 bins of an image nobody settled (a kernel's output): every pixel the truth decides is counted in
    its bin, every ambiguous one in one of the two bins at its edge — decided exactly, bin by bin from 0 up: x pixels of those
    between b and b + 1 are counted in b + 1, and 0 <= x <= their number must hold at every b.  An image without ambiguous pixels
    must give the float64 counts exactly.  Returns (ambiguous pixels, pixels counted on the other side of their edge than float64)."""
    lo, hi = bin_choices(image, min_log, log_range)
    fixed = hist_of(lo[lo == hi]).astype(np.int64)
    flex = hist_of(lo[lo != hi]).astype(np.int64)
    assert ((hi - lo) >= 0).all() and ((hi - lo) <= 1).all() and flex[255] == 0
    got = np.asarray(got_hist).astype(np.int64).reshape(-1) & 0xFFFFFFFF
    want = hist_of(image_bins(image, min_log, log_range)[0]).astype(np.int64)
    x = 0
    for b in range(256):
        x = fixed[b] + flex[b] + x - got[b]                          # of the pixels between b and b + 1, those counted in b + 1
        assert 0 <= x <= flex[b], (f"bin {b}: got {got[b]}, the truth decides {fixed[b]} and leaves {flex[b]} to bins {b} | {b + 1}; "
                                   f"float64 counts {want[max(b - 1, 0):b + 2].tolist()}, got {got[max(b - 1, 0):b + 2].tolist()}")
    return int(flex.sum()), int(np.abs(got - want).sum()) // 2


# ---------------------------------------------------------------------------------------------------------------- tone-map
ACES = (2.51, 0.03, 2.43, 0.59, 0.14)   # hdr_tone_mapping.hlsl:27-36


def _v_of_m(m):
    with np.errstate(all="ignore"):
        gc = np.where(m > 0.0, np.power(np.clip(m, 0.0, 1.0), 0.454545), 0.0)
    return np.clip(gc, 0.0, 1.0) * 255.0 + 0.5


def _aces_terms(c, avg):
    a, b, cc, d, e = ACES
    with np.errstate(all="ignore"):
        x = c / (9.6 * float(np.float32(avg)) + 0.001)
        t1 = a * x + b
        num = x * t1
        t2 = cc * x + d
        den = x * t2 + e
    return x, t1, num, t2, den


def tonemap_truth(rgb, avg):
    """(v, byte, ambiguous, finite) per channel of rgb [..., 3] (half values): v the unrounded channel value, byte = floor(v) (0 for a
    non-finite channel: Inf / Inf = NaN and saturate(NaN) = 0), ambiguous where v is within DELTA_T of an integer."""
    c = np.asarray(rgb).astype(np.float64)
    finite = np.isfinite(c)
    x, _, num, _, den = _aces_terms(np.where(finite, c, 0.0), avg)
    m = np.where(finite, np.clip(num / den, 0.0, 1.0), 0.0)
    v = _v_of_m(m)
    byte = np.floor(v).astype(np.int64)
    amb = finite & (np.abs(v - np.rint(v)) <= DELTA_T)
    return v, byte, amb, finite


def tonemap_band(rgb, avg):
    """the derived error bound of v in LSB per channel (module docstring); 0 for non-finite channels"""
    a, b, cc, d, e = ACES
    c = np.asarray(rgb).astype(np.float64)
    finite = np.isfinite(c)
    x, t1, num, t2, den = _aces_terms(np.where(finite, c, 0.0), avg)
    ex = 6 * U
    ax = np.abs(x)
    with np.errstate(all="ignore"):
        e_t1 = a * ax * (2 * U + ex) + b * U + U * np.abs(t1)
        e_num = ax * e_t1 + np.abs(num) * (ex + U)
        e_t2 = cc * ax * (2 * U + ex) + d * U + U * np.abs(t2)
        e_p = np.abs(x * t2) * (ex + U) + ax * e_t2
        e_den = e_p + e * U + U * np.abs(den)
        q = num / den
        e_q = e_num / den + np.abs(q) * (e_den / den + 3 * U)
        v = _v_of_m(np.clip(q, 0.0, 1.0))
        spread = np.maximum(_v_of_m(np.clip(q + e_q, 0.0, 1.0)) - v, v - _v_of_m(np.clip(q - e_q, 0.0, 1.0)))
        gc = (v - 0.5) / 255.0
        lg = np.where(gc > 0.0, np.abs(np.log2(np.maximum(gc, 1e-300))) / 0.454545, 0.0)
        post = 255.0 * gc * (1.26 * lg + 2.0) * U + 256 * U
    return np.where(finite, spread + post, 0.0)


def unpack(rgba8):
    """[h, w] uint32 -> ([h, w, 3] int64 bytes R, G, B; [h, w] alpha)"""
    p = np.asarray(rgba8).astype(np.int64) & 0xFFFFFFFF
    return np.stack([(p >> (8 * k)) & 255 for k in range(3)], axis=-1), p >> 24


def check_ldr(got_rgba8, image, avg):
    """The assertions on a tone-mapped image got [h, w] uint32 of image [h, w, 4] half at adapted luminance avg.  Returns
    {"left_out", "cases", "max_excess"}: max_excess is how far outside [byte, byte + 1) the float64 v lies at worst, i.e. the smallest
    error the implementation can have made."""
    got, alpha = unpack(got_rgba8)
    v, want, amb, finite = tonemap_truth(image[..., :3], avg)
    assert got.shape == want.shape
    assert np.all(alpha == 255), "alpha"
    assert np.all(got[~finite] == 0), "a non-finite channel must give 0"
    d = np.abs(got - want)
    assert d.max() <= 1, f"a byte is {d.max()} from floor(v)"
    wrong = (d != 0) & ~amb
    if wrong.any():
        i = tuple(np.argwhere(wrong)[0])
        raise AssertionError(f"{int(wrong.sum())} unambiguous channels differ; first at {i}: value {float(image[i[0], i[1], i[2]])!r} "
                             f"avg {avg!r} v {v[i]!r} got {got[i]} want {want[i]}")
    excess = np.where(got > want, got - v, np.where(got < want, v - (got + 1), 0.0))
    return {"left_out": int(amb.sum()), "cases": int(finite.sum()), "max_excess": float(excess.max())}


def check_monotone(got_rgba8):
    """all_halves_rgb's R channel holds pattern i at pixel i: over the non-negative finite halves (patterns 0 .. 0x7BFF, increasing) the
    R byte must not decrease — the ACES curve's derivative has the numerator 1.408 x^2 + 0.7028 x + 0.0042 > 0 for x >= 0"""
    red = unpack(got_rgba8)[0][..., 0].reshape(-1)[:0x7C00]
    assert np.all(np.diff(red) >= 0), "tone-map not monotone in the input"


# ---------------------------------------------------------------------------------------------------------------- average
def _fp32_exact(x):
    return float(np.float32(x)) == float(x)


def average_truth(hist, pixel_count, dt, prev, min_log=MIN_LOG, log_range=LOG_RANGE):
    """hdr_average_histogram.hlsl:26-73 in float64, quirks kept.  Returns a dict: result, avg_bin (unfloored), bin, lum, tt, band (the
    absolute band of avg_bin: 0 where every fp32 step is exact), ambiguous (an integer >= 1 lies within the band of avg_bin)."""
    hist = np.asarray(hist).astype(np.uint64).reshape(256)
    prod = (hist * np.arange(256, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)      # quirk: count * index is a uint32 product and wraps
    terms = prod.astype(np.float64)
    exact = all(_fp32_exact(t) for t in terms)
    level = terms.copy()
    step = 128
    while step:                                                                  # the shader's LDS tree, to see whether fp32 rounds in it
        level = level[:step] + level[step:2 * step]
        exact = exact and all(_fp32_exact(t) for t in level)
        step >>= 1
    total = float(terms.sum())                                                   # exact in float64 (< 2^40)
    den = (int(pixel_count) - int(hist[0])) & 0xFFFFFFFF                         # quirk: divides by pixel_count - hist[0], uint32
    with np.errstate(all="ignore"):
        avg_bin = float(np.float64(total) / np.float64(den))                     # 0 / 0 = NaN on an all-black frame
    exact = exact and _fp32_exact(den) and np.isfinite(avg_bin) and _fp32_exact(avg_bin) and avg_bin * den == total
    if not (avg_bin == avg_bin and avg_bin > 0.0):
        b = 0                                                                    # quirk: float -> uint conversion; NaN / negative -> 0
    elif avg_bin >= 4294967296.0:
        b = 0xFFFFFFFF
    else:
        b = int(avg_bin)                                                         # quirk: truncation, not rounding
    band = 0.0 if exact or not np.isfinite(avg_bin) else avg_bin * AVG_BIN_REL
    near = float(np.rint(avg_bin)) if np.isfinite(avg_bin) else 0.0
    ambiguous = bool(np.isfinite(avg_bin) and band > 0.0 and near >= 1.0 and abs(avg_bin - near) <= band)
    with np.errstate(all="ignore"):
        lum = float(np.exp2(np.float64((b - 1.0) / 254.0 * log_range + min_log)))
        tt = float(np.clip(1.0 - np.exp(-float(np.float32(dt)) * 1.6), 0.0, 1.0))   # SMOOTH_TIME 1.6; exponential blend
    p = float(np.float32(prev))
    return dict(result=p + tt * (lum - p), avg_bin=avg_bin, bin=b, lum=lum, tt=tt, band=band, ambiguous=ambiguous, prev=p, near=int(near))


def bin_luminance(b, min_log=MIN_LOG, log_range=LOG_RANGE):
    return float(np.exp2((b - 1.0) / 254.0 * log_range + min_log))


def blend_bound(lum, prev, tt, dt):
    """absolute fp32 bound of prev + tt * (lum - prev) (module docstring)"""
    arg = abs(float(np.float32(dt)) * 1.6)
    e_tt = 0.0 if tt >= 1.0 and arg > 20.0 else 2 * U * max(1.0 - tt, 2.0 ** -126) + arg * 2 * U * (1.0 - tt)
    diff = abs(lum - prev)
    result = abs(prev + tt * (lum - prev))
    return diff * e_tt + tt * (lum * LUM_REL + diff * 2 * U) + U * result


def check_average(got, hist, pixel_count, dt, prev, min_log=MIN_LOG, log_range=LOG_RANGE):
    """got (fp32 adapted luminance) against average_truth.  Where the truncation is ambiguous either neighbouring bin is accepted (and
    the caller counts it).  Returns (ambiguous, relative error against the accepted value)."""
    t = average_truth(hist, pixel_count, dt, prev, min_log, log_range)
    bins = [t["bin"]] if not t["ambiguous"] else [t["near"] - 1, t["near"]]
    best = None
    for b in bins:
        lum = bin_luminance(b, min_log, log_range)
        want = t["prev"] + t["tt"] * (lum - t["prev"])
        bound = blend_bound(lum, t["prev"], t["tt"], dt)
        err = abs(float(got) - want)
        if best is None or err - bound < best[0] - best[1]:
            best = (err, bound, want)
    err, bound, want = best
    assert err <= bound, f"average: got {float(got)!r} want {want!r} (bin {bins}, avg_bin {t['avg_bin']!r}): off by {err:.3e}, bound {bound:.3e}"
    return t["ambiguous"], err / abs(want) if want else 0.0


def average_histograms(n=200, seed=0x5EED17):
    """n seeded (hist uint32 [256], pixel_count): 4K frames of several shapes, one-bin and two-bin frames, all black but one pixel, and
    the uint32-wrap case.  Asserts the cap on ambiguous truncations."""
    rng = np.random.default_rng(seed)
    px4k = 3840 * 2160
    out = []
    wrap = np.zeros(256, np.uint32)
    wrap[255] = 20_000_000                                                       # 20e6 * 255 > 2^32
    out.append((wrap, 20_000_000))
    for b in (1, 2, 100, 254, 255):                                              # one-bin frames
        h = np.zeros(256, np.uint32)
        h[b] = px4k
        out.append((h, px4k))
    for b in (1, 77, 255):                                                       # black but one pixel
        h = np.zeros(256, np.uint32)
        h[0], h[b] = px4k - 1, 1
        out.append((h, px4k))
    for _ in range(20):                                                          # two-bin frames
        b1, b2 = rng.choice(np.arange(1, 256), 2, replace=False)
        n1 = int(rng.integers(1, px4k))
        h = np.zeros(256, np.uint32)
        h[b1], h[b2] = n1, px4k - n1
        out.append((h, px4k))
    while len(out) < n:
        kind = len(out) % 4
        if kind == 0:                                                            # a lobe around a centre bin, some black
            centre, width = rng.uniform(5, 250), rng.uniform(1, 40)
            p = np.exp(-0.5 * ((np.arange(256) - centre) / width) ** 2)
            p[0] = rng.uniform(0, 0.3) * p.sum()
        elif kind == 1:                                                          # flat noise
            p = rng.uniform(0, 1, 256)
        elif kind == 2:                                                          # a few populated bins
            p = np.zeros(256)
            p[rng.choice(256, int(rng.integers(3, 9)), replace=False)] = rng.uniform(0.1, 1, 1)
        else:                                                                    # small frames of odd pixel counts
            p = rng.uniform(0, 1, 256) ** 8
        count = px4k if kind != 3 else int(rng.integers(1, 100_000))
        h = rng.multinomial(count, p / p.sum()).astype(np.uint32)
        if h[0] == count:
            h[0] -= 1
            h[200] += 1
        out.append((h, count))
    amb = sum(average_truth(h, c, 1e9, 0.0)["ambiguous"] for h, c in out)
    assert amb <= AVERAGE_CAP * len(out), f"{amb} of {len(out)} histograms truncate ambiguously: above the cap"
    return out


# ---------------------------------------------------------------------------------------------------------------- case builders
def _halves(patterns):
    return np.asarray(patterns, dtype=np.uint16).view(np.float16)


def _image(r, g, b, w=256):
    img = np.ones((r.size // w, w, 4), dtype=np.float16)
    for k, c in enumerate((r, g, b)):
        img[..., k] = c.reshape(-1, w)
    return img


def all_halves_grey_raw():
    p = _halves(np.arange(65536))
    return _image(p, p, p)


def all_halves_grey(min_log=MIN_LOG, log_range=LOG_RANGE):
    """the 65 536 half bit patterns as r = g = b, 256 x 256, ambiguous pixels replaced by black: (image, replaced, closest edge kept)"""
    return settle(all_halves_grey_raw(), min_log, log_range)


def finite_halves_grey():
    """all_halves_grey() with Inf and NaN black too (what a bloom pass can carry through unchanged)"""
    img, n, dist = all_halves_grey()
    img[~np.isfinite(img[..., 0].astype(np.float32)), :3] = 0
    return img, n, dist


def _bit_reverse16(x):
    x = np.asarray(x, dtype=np.uint32)
    r = np.zeros_like(x)
    for k in range(16):
        r |= ((x >> k) & 1) << (15 - k)
    return r


def all_halves_rgb():
    """R = pattern i, G = pattern i * 40503 mod 65536, B = that one bit-reversed: every channel sees every half, a channel swap or a
    swap of the two pixels of a pair changes the answer, and Inf / NaN share pixels and pairs with finite values"""
    i = np.arange(65536, dtype=np.uint32)
    gp = (i * 40503) & 0xFFFF
    img = _image(_halves(i), _halves(gp), _halves(_bit_reverse16(gp)))
    fin = np.isfinite(img[..., :3].astype(np.float32))
    mixed = ~fin.all(-1) & fin.any(-1)
    pair_mixed = ~fin.all(-1)[:, 0::2] & fin.all(-1)[:, 1::2]
    assert mixed.sum() > 1000 and pair_mixed.sum() > 1000
    return img


def colour_triples(n=65536, seed=0xC0104, min_log=MIN_LOG, log_range=LOG_RANGE):
    """log-uniform in [2^-26, 2^16) per channel, cast to half (subnormals, zeros and overflow to Inf included), n / 256 x 256, settled"""
    rng = np.random.default_rng(seed)
    with np.errstate(over="ignore"):
        c = np.exp2(rng.uniform(-26.0, 16.0, (3, n))).astype(np.float16)
    return settle(_image(c[0], c[1], c[2]), min_log, log_range)


def bin_centre(b):
    """the half nearest the centre of bin b (1 .. 254) at the default range; 0 -> black, 255 -> 8.0"""
    if b == 0:
        return np.float16(0.0)
    if b == 255:
        return np.float16(8.0)
    return np.float16(2.0 ** (((b - 0.5) / 254.0) * LOG_RANGE + MIN_LOG))


BIN_CENTRES = np.array([bin_centre(b) for b in range(256)], dtype=np.float16)
assert np.array_equal(bin_truth(BIN_CENTRES, BIN_CENTRES, BIN_CENTRES)[0], np.arange(256))
assert not bin_truth(BIN_CENTRES, BIN_CENTRES, BIN_CENTRES)[1].any()


def grey_frame(bins):
    """[h, w] bin indices -> [h, w, 4] half frame of those bins' centre values (alpha 1)"""
    bins = np.asarray(bins)
    img = np.ones(bins.shape + (4,), dtype=np.float16)
    img[..., :3] = BIN_CENTRES[bins][..., None]
    return img


def end_to_end_range(b):
    """where histogram + average (dt = 1e9, prev = 0) must put a constant frame of bin_centre(b): the average reconstructs the lower
    edge of the value's bin, so [L 2^(-range/254), L] widened by LUM_REL; the clamped frame (b = 255) gives the top bin's value"""
    if b == 255:
        top = bin_luminance(255)
        return top * (1 - LUM_REL), top * (1 + LUM_REL)
    lum = float(bin_centre(b))
    return lum * 2.0 ** (-LOG_RANGE / 254.0) * (1 - LUM_REL), lum * (1 + LUM_REL)


def tile_to(img, w, h):
    """img repeated to w x h"""
    ry, rx = -(-h // img.shape[0]), -(-w // img.shape[1])
    return np.ascontiguousarray(np.tile(img, (ry, rx, 1))[:h, :w])
