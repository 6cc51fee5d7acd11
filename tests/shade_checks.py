"""The shade's parity checks, shared by the test modules that compare a shaded image with the CPU oracle and the double-precision
truth (test_gpu_parity.py, test_gpu_cameras.py, test_cameras_cpu.py): the bounds of DESIGN.md section 2, stated once."""
import numpy as np

import common

def assert_half_close(got, want, max_ulp, what, frac_over=0.0, hard_ulp=None):
    d = common.half_ulp_diff(got, want)
    nan_mismatch = np.isnan(got.astype(np.float32)) != np.isnan(want.astype(np.float32))
    assert not nan_mismatch.any(), f"{what}: NaN pattern differs"
    over = (d > max_ulp) & ~np.isnan(want.astype(np.float32))
    assert over.mean() <= frac_over, f"{what}: {over.sum()} of {d.size} texels differ by > {max_ulp} ULP (max {d.max()})"
    if hard_ulp is not None:
        assert d[~np.isnan(want.astype(np.float32))].max() <= hard_ulp, f"{what}: max ULP {d.max()} > {hard_ulp}"


F64_ORACLE_FACTOR = 4.0     # a pixel may be this many times further from the exact value than the fp32 restatement is ...
F32_REL_LINF = 1e-4         # ... on top of the relative L-inf bound north_star states
# ... but the measured term is CAPPED where the formula is known to be tame: at roughness >= 48/255 (the bench range; a^4 >= 1.2e-3) the
# restatement's own distance has never exceeded 6.2e-4 of scale, so an allowance above 1e-3 there would mean the
# restatement — the builder's own code, which widens the bound with its error — has regressed, not that the pixel is hard
MEASURED_TERM_CAP = 1e-3
ROUGH_TAME = 48
FLAG_CLUSTER_EDGE = 4       # orc_deferred_shade_f64: the cluster slice / column / row of the pixel is within rounding of an edge
PARITY_LOG = []             # (what, comparable fraction, well-conditioned fraction, worst ratio): printed by the tests, asserted below


def _truth_bound(orc, want_f32, truth, on, rough=None, decided=False):
    """Per-pixel, per-channel allowance of the parity bound: 1e-4 * scale + 4 * |oracle_f32 - f64|.  The second term is
    measured, not modelled: where the reference formula is ill-conditioned in fp32 (GGX highlights: t = NdotH^2 (a^4 - 1) + 1
    cancels) the fp32 restatement itself is that far from the exact value, and the GPU may be as well — but not more than
    a small factor further.  Returns (bound, scale, comparable-pixel mask over the `on` pixels).
    decided: the truth takes the pixel's cluster from the oracle's fp32 decision and only FLAGS (4) the pixels whose slice, column or
    row is decided by rounding, so its interval holds for the oracle's cluster there too; an image that is contracted to take the
    oracle's cluster to the bit (the kernel's slice, column and row are) is comparable on those pixels as well.  Flags 1 (stencil) and 2
    (octahedral fold) stay excluded."""
    lo, hi, flags = truth
    ok = ((flags & ~np.uint8(FLAG_CLUSTER_EDGE) if decided else flags) == 0)[on]
    scale = float(np.abs(hi[on][ok]).max())
    d_orc = orc.truth_distance(want_f32, lo, hi)[on]
    measured = F64_ORACLE_FACTOR * d_orc
    if rough is not None:
        tame = (np.asarray(rough)[on] >= ROUGH_TAME)[:, None]
        measured = np.where(tame, np.minimum(measured, MEASURED_TERM_CAP * scale), measured)
    return F32_REL_LINF * scale + measured, scale, ok, d_orc


def _check_shade(orc, got, want, want_f32, truth, stencil, what, hard_ulp=64, rough=None, decided=False):
    """The fp16 target.  (1) Against the double-precision truth: every comparable pixel within
    1e-4 * scale + 4 * |oracle_f32 - f64| of the exact value, plus the fp16 rounding of the stored value (half an ulp of
    the value itself).  (2) Against the fp32 restatement's fp16 image, in ULPs, on the well-conditioned pixels (those where
    the restatement is within a quarter of the bound of the exact value)."""
    on = stencil > 0
    lo, hi, flags = truth
    bound, scale, ok, d_orc = _truth_bound(orc, want_f32, truth, on, rough, decided)
    assert ok.mean() >= 0.95, f"{what}: only {ok.mean():.3f} of the pixels are comparable with the truth"
    g32 = got.astype(np.float32)
    dist = orc.truth_distance(g32, lo, hi)[on]
    store = np.abs(g32[on][:, :3]).astype(np.float64) * 2.0 ** -11 + 2.0 ** -25      # round-to-nearest of the half store (+ half a subnormal step)
    worst = (dist / (bound + store))[ok]
    assert (worst <= 1.0).all(), f"{what}: a pixel is {worst.max():.2f} x its bound from the exact value (scale {scale})"
    # pixels on a cluster / octahedral-fold edge have no truth to compare with: against the fp32 restatement, all but a handful
    # (an evaluation that lands on the other side of the edge walks another light list)
    err = np.abs(g32 - want.astype(np.float32))[on][:, :3]
    off = (err > F32_REL_LINF * scale + scale * 2.0 ** -10 + F64_ORACLE_FACTOR * d_orc).any(axis=1) & ~ok
    assert off.sum() <= max(2, int(1e-4 * on.sum())), f"{what}: {int(off.sum())} edge pixels differ from the fp32 restatement"
    well = ok & (d_orc.max(axis=1) <= 0.25 * F32_REL_LINF * scale)
    assert well.mean() >= 0.97, f"{what}: only {well.mean():.3f} of the pixels are well-conditioned"
    PARITY_LOG.append((what, float(ok.mean()), float(well.mean()), float(worst.max())))
    print(f"[parity] {what}: comparable with the f64 truth {ok.mean():.4f}, well-conditioned {well.mean():.4f}, worst pixel {worst.max():.2f} x its bound", flush=True)
    # hard_ulp bounds the RELATIVE error of every channel; on a million-texel band a near-black channel (absolute error
    # still inside the L-inf bound above) can exceed it, so the full-size tests pass None
    assert_half_close(got[on][well], want[on][well], 2, what, frac_over=1e-3, hard_ulp=hard_ulp)
    assert np.all(got[on][:, 3] == 1.0)


def _check_shade_f32(orc, got, want_f32, truth, stencil, what, rough=None, decided=False):
    """Per pixel and channel: |gpu_f32 - f64| <= 1e-4 * scale + 4 * |oracle_f32 - f64|, where f64 is the double-precision
    evaluation of the reference's formulas on the same inputs (an interval where a sampler snap / face choice is decided by
    rounding) and scale = max |f64| over the covered pixels.  No term of the bound is modelled: the fp32 restatement's own
    distance to the exact value is measured, and the GPU gets a small multiple of it.  Edge pixels (cluster cell / octahedral
    fold decided by rounding: no single truth) are compared with the fp32 restatement instead, all but a handful.
    Returns the two error distributions (gpu, oracle; relative to scale) for the report in DESIGN.md section 2."""
    on = stencil > 0
    lo, hi, flags = truth
    assert np.isfinite(got[on][:, :3]).all() and np.isfinite(want_f32[on][:, :3]).all(), what
    bound, scale, ok, d_orc = _truth_bound(orc, want_f32, truth, on, rough, decided)
    assert ok.mean() >= 0.95, f"{what}: only {ok.mean():.3f} of the pixels are comparable with the truth"
    print(f"[parity] {what} (fp32): comparable with the f64 truth {ok.mean():.4f}", flush=True)
    d_gpu = orc.truth_distance(got, lo, hi)[on]
    worst = (d_gpu / bound)[ok]
    assert (worst <= 1.0).all(), \
        f"{what}: a pixel is {worst.max():.2f} x its bound from the exact value (gpu {d_gpu[ok].max() / scale:.3g}, oracle {d_orc[ok].max() / scale:.3g} of scale)"
    err = np.abs(got[on][:, :3].astype(np.float64) - want_f32[on][:, :3])
    off = (err > bound).any(axis=1) & ~ok
    assert off.sum() <= max(2, int(1e-4 * on.sum())), f"{what}: {int(off.sum())} edge pixels differ from the fp32 restatement"
    # not SYSTEMATICALLY further from the truth than the restatement: the upper quantiles of the two distributions agree
    rg, ro = d_gpu[ok].max(axis=1) / scale, d_orc[ok].max(axis=1) / scale
    for q in (0.99, 0.999, 0.9999):
        assert np.quantile(rg, q) <= 2.0 * np.quantile(ro, q) + 2e-6, f"{what}: gpu q{q} {np.quantile(rg, q):.3g} vs oracle {np.quantile(ro, q):.3g}"
    assert np.all(got[on][:, 3] == 1.0)
    return rg, ro
