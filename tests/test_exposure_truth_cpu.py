"""The CPU oracle's exposure functions under the float64 truth of tests/exposure_truth.py: the same case sets and assertions
tests/test_gpu_exposure_truth.py applies to the kernels, so the reference alone is shown to stay inside the derived bands and the
caps on what a case set may leave out — and the case sets to reach all 256 bins and all 256 output bytes."""
import ctypes as C

import numpy as np
import pytest

import exposure_truth as et


def orc_histogram(orc, image, min_log=et.MIN_LOG, log_range=et.LOG_RANGE, times=1):
    h, w = image.shape[:2]
    image = np.ascontiguousarray(image)
    hist = np.zeros(256, dtype=np.uint32)
    for _ in range(times):
        st = orc.lib().orc_lum_histogram(image.ctypes.data_as(C.c_void_p), w, h, w, min_log, float(np.float32(1.0) / np.float32(log_range)),
                                         hist.ctypes.data_as(C.c_void_p))
        assert st == 0
    return hist


def test_bands_are_the_derived_ones():
    assert 1.0e-4 < et.delta_h_bound() < et.DELTA_H < 2 * 1.3e-4 and et.delta_h_bound(-6.0, 8.0) < et.DELTA_H
    rgb = et.all_halves_rgb()[..., :3]
    worst = max(float(et.tonemap_band(rgb, avg).max()) for avg in et.TONEMAP_LUMS)
    nonneg = np.where(rgb.astype(np.float32) >= 0, rgb, np.float16(0))
    worst_pos = max(float(et.tonemap_band(nonneg, avg).max()) for avg in et.TONEMAP_LUMS)
    print(f"tonemap_band: max {worst:.3e} LSB, non-negative inputs {worst_pos:.3e}")
    assert et.DELTA_T / 2 < worst < et.DELTA_T and worst_pos < et.DELTA_T / 2


def test_bin_truth_conventions():
    h = np.float16
    r = np.array([0.0, -1.0, np.nan, np.inf, -np.inf, 1e-3, 8.0, 6e-8], dtype=h)
    bins, amb, _ = et.bin_truth(r, r, r)
    # black, negative and -Inf are below 1e-6: bin 0; NaN takes the log branch and saturate(NaN) = 0: bin 1; +Inf clamps to 255
    assert bins.tolist() == [0, 0, 1, 255, 0, int(np.floor((np.log2(float(h(1e-3))) + 10) / 12 * 254 + 1)), 255, 0] and not amb.any()
    edge = 2.0 ** ((99.0 / 254.0) * 12 - 10)                                     # the edge between bins 99 and 100
    b, a, d = et.bin_truth(np.float64(edge), np.float64(edge), np.float64(edge))
    assert a and d < 1e-9
    b, a, _ = et.bin_truth(np.float64(1e-6), np.float64(1e-6), np.float64(1e-6))
    assert a


@pytest.mark.parametrize("case", ["grey", "triples", "grey_other_range", "triples_4x"])
def test_oracle_histogram_every_half_value(orc, case):
    ml, lr = (-6.0, 8.0) if case == "grey_other_range" else (et.MIN_LOG, et.LOG_RANGE)
    if case.startswith("grey"):
        img, replaced, closest = et.all_halves_grey(ml, lr)
    else:
        img, replaced, closest = et.colour_triples(65536 * (4 if case == "triples_4x" else 1), min_log=ml, log_range=lr)
    n = img.shape[0] * img.shape[1]
    print(f"{case}: {replaced} of {n} replaced as ambiguous, closest edge kept {closest:.3e} bins")
    assert replaced <= et.HIST_CAP * n
    want = et.hist_of(et.image_bins(img, ml, lr)[0])
    assert np.all(want > 0), "the case set must reach all 256 bins"
    et.check_histogram(orc_histogram(orc, img, ml, lr, times=2), img, ml, lr, times=2)


def fp32_histogram(image, log_error=0.0, swap=False):
    """the shader's arithmetic in numpy float32 (optionally with a relative error in log2, or R and B swapped)"""
    f = np.float32
    c = image.astype(f)
    r, g, b = (c[..., 2], c[..., 1], c[..., 0]) if swap else (c[..., 0], c[..., 1], c[..., 2])
    with np.errstate(all="ignore"):
        lum = (r * f(0.2126) + g * f(0.7152)) + b * f(0.0722)
        lg = np.log2(lum) * f(1.0 + log_error)
        t = (lg - f(et.MIN_LOG)) * (f(1.0) / f(et.LOG_RANGE))
        s = np.where(np.isnan(t), f(0), np.clip(t, f(0), f(1)))
        bins = np.where(lum < f(et.EPSILON), 0, np.floor(s * f(254.0) + f(1.0))).astype(np.int64)
    return et.hist_of(bins)


def test_the_checks_have_teeth(orc):
    """an fp32 restatement in numpy passes; a log2 good to 2^-16 only, swapped channels, one pixel counted in the neighbouring bin and
    one tone-mapped channel one LSB off all fail"""
    grey, triples = et.all_halves_grey()[0], et.colour_triples()[0]
    for img in (grey, triples):
        et.check_histogram(fp32_histogram(img), img)
        with pytest.raises(AssertionError):
            et.check_histogram(fp32_histogram(img, log_error=2.0 ** -16), img)
        moved = fp32_histogram(img)
        moved[100] -= 1
        moved[101] += 1
        with pytest.raises(AssertionError):
            et.check_histogram(moved, img)
    with pytest.raises(AssertionError):
        et.check_histogram(fp32_histogram(triples, swap=True), triples)
    img = et.all_halves_rgb()
    good = orc.tonemap(img, 0.18)
    v, byte, amb, finite = et.tonemap_truth(img[..., :3], 0.18)
    y, x, k = np.argwhere(finite & ~amb & (byte > 0) & (byte < 255))[1234]
    bad = good.copy()
    bad[y, x] += np.uint32(1 << (8 * k))
    with pytest.raises(AssertionError):
        et.check_ldr(bad, img, 0.18)
    swapped = (good & np.uint32(0xFF00FF00)) | ((good & np.uint32(0xFF)) << np.uint32(16)) | ((good >> np.uint32(16)) & np.uint32(0xFF))
    with pytest.raises(AssertionError):
        et.check_ldr(swapped, img, 0.18)
    pair = good.copy()
    pair[:, 0::2], pair[:, 1::2] = good[:, 1::2], good[:, 0::2]
    with pytest.raises(AssertionError):
        et.check_ldr(pair, img, 0.18)


def test_finite_halves_and_patterned_frames(orc):
    img, _, _ = et.finite_halves_grey()
    assert np.isfinite(img.astype(np.float32)).all()
    et.check_histogram(orc_histogram(orc, img), img)
    yy, xx = np.mgrid[0:5, 0:514]
    frame = et.grey_frame(1 + (xx * 7 + yy * 13) % 254)
    et.check_histogram(orc_histogram(orc, frame), frame)
    assert np.array_equal(et.hist_of(et.image_bins(et.grey_frame(np.arange(256)[None]))[0]), np.ones(256, np.uint32))


def test_oracle_tonemap_every_half_value(orc):
    img = et.all_halves_rgb()
    left, cases, seen, worst = 0, 0, np.zeros(256, bool), 0.0
    for avg in et.TONEMAP_LUMS:
        got = orc.tonemap(img, avg)
        st = et.check_ldr(got, img, avg)
        et.check_monotone(got)
        left, cases, worst = left + st["left_out"], cases + st["cases"], max(worst, st["max_excess"])
        v, byte, amb, finite = et.tonemap_truth(img[..., :3], avg)
        seen[np.unique(byte[finite & ~amb])] = True
    print(f"tone-map: {left} of {cases} (value, luminance) cases left out ({100.0 * left / cases:.3f} %), oracle max excess {worst:.3e} LSB")
    assert left <= et.TONEMAP_CAP * cases
    assert seen.all(), "the case set must reach all 256 output bytes"


def test_tonemap_truth_conventions():
    img = np.ones((1, 6, 4), dtype=np.float16)
    img[0, :, :3] = np.array([[np.inf, 0.5, 0.5], [0.5, np.nan, 0.5], [-np.inf, 0, 0], [-0.0117, -0.0121, 0.0], [65504, 65504, 65504], [-1, -1, -1]])
    v, byte, amb, finite = et.tonemap_truth(img[..., :3], 0.104)                  # x = c / 0.9994...
    assert byte[0, 0, 0] == 0 and byte[0, 1, 1] == 0 and byte[0, 2, 0] == 0 and byte[0, 0, 1] == byte[0, 1, 0] > 100
    assert byte[0, 3, 0] == 0 and byte[0, 3, 1] > 0          # either side of the numerator's zero crossing at x = -0.01195
    assert byte[0, 4].tolist() == [255] * 3 and byte[0, 5].tolist() == [255] * 3 and byte[0, 3, 2] == 0


def test_oracle_average(orc):
    cases = et.average_histograms()
    assert len(cases) == 200
    amb = 0
    worst = 0.0
    for hist, count in cases:
        a, rel = et.check_average(orc.lum_average(hist.copy(), count, 1e9, 0.0), hist, count, 1e9, 0.0)
        amb += a
        worst = max(worst, rel)
        _, rel = et.check_average(orc.lum_average(hist.copy(), count, 1.0 / 60.0, 0.18), hist, count, 1.0 / 60.0, 0.18)
        worst = max(worst, rel)
    print(f"average: {amb} of {len(cases)} ambiguous truncations, oracle worst relative error {worst:.3e}")
    assert amb <= et.AVERAGE_CAP * len(cases)


def test_average_truth_quirks(orc):
    h = np.zeros(256, np.uint32)
    h[10], h[11] = 1, 3
    t = et.average_truth(h, 4, 1e9, 0.0)
    assert t["avg_bin"] == 10.75 and t["bin"] == 10 and not t["ambiguous"]       # truncation
    h = np.zeros(256, np.uint32)
    h[255] = 20_000_000
    t = et.average_truth(h, 20_000_000, 1e9, 0.0)
    assert t["avg_bin"] == pytest.approx(((20_000_000 * 255) % 2 ** 32) / 20_000_000) and t["avg_bin"] < 41   # the uint32 wrap
    assert t["avg_bin"] == pytest.approx(orc.lum_average_bin(h, 20_000_000), rel=et.AVG_BIN_REL)
    h = np.zeros(256, np.uint32)
    h[0], h[200] = 99, 1
    assert et.average_truth(h, 100, 1e9, 0.0)["bin"] == 200                      # black pixels leave the denominator
    h[0], h[200] = 100, 0
    t = et.average_truth(h, 100, 1.0 / 60.0, 0.25)
    assert np.isnan(t["avg_bin"]) and t["bin"] == 0                              # 0 / 0 -> bin 0
    h = np.zeros(256, np.uint32)
    h[100] = 3840 * 2160
    t = et.average_truth(h, 3840 * 2160, 1e9, 0.0)
    assert t["band"] == 0.0 and t["bin"] == 100 and not t["ambiguous"]           # every fp32 step exact: decided


def test_end_to_end_constant_frames(orc):
    for b in (1, 2, 64, 128, 254, 255):
        frame = et.grey_frame(np.full((64, 64), b))
        hist = orc_histogram(orc, frame)
        et.check_histogram(hist, frame)
        avg = orc.lum_average(hist.copy(), 64 * 64, 1e9, 0.0)
        lo, hi = et.end_to_end_range(b)
        assert lo <= avg <= hi, (b, avg, lo, hi)
        et.check_ldr(orc.tonemap(frame, avg), frame, avg)


# ------------------------------------------------------------------------------------------------------ a kernel's output, not settled
def test_histogram_of_an_output_is_exact_where_the_truth_decides():
    """check_histogram_of_output on every positive finite grey half: the float64 counts pass; an ambiguous pixel counted on the other
    side of its edge passes and is reported; a pixel the truth decides counted in the next bin is rejected, and so is an ambiguous
    pixel counted anywhere but at its edge"""
    p = et._halves(np.arange(1, 0x7C00))
    p = p[:p.size // 256 * 256]
    img = et._image(p, p, p)
    bins, amb, _ = et.image_bins(img)
    lo, hi = et.bin_choices(img)
    assert amb.any() and ((lo != hi) == amb).all() and ((bins == lo) | (bins == hi)).all()
    want = et.hist_of(bins).astype(np.int64)
    assert et.check_histogram_of_output(want, img) == (int(amb.sum()), 0)
    b = int(bins[amb][0])
    other = int((lo + hi)[amb][0]) - b
    moved = want.copy()
    moved[b] -= 1
    moved[other] += 1
    assert et.check_histogram_of_output(moved, img) == (int(amb.sum()), 1)
    far = want.copy()
    far[b] -= 1
    far[b + 3] += 1
    with pytest.raises(AssertionError, match="the truth decides"):
        et.check_histogram_of_output(far, img)
    flex = et.hist_of(lo[amb])                                       # an edge no ambiguous pixel sits at: bins d | d + 1 both populated, decided
    d = next(k for k in range(2, 254) if flex[k] == 0 and want[k] > 0)
    wrong = want.copy()
    wrong[d] -= 1
    wrong[d + 1] += 1
    with pytest.raises(AssertionError, match="the truth decides"):
        et.check_histogram_of_output(wrong, img)
