"""The CPU oracle's SH9 projection and diffuse evaluation under the float64 truth of tests/sh9_truth.py: the same skies, bands and
assertions tests/test_gpu_sh9_truth.py applies to the kernels; the truth's own analytic closure (second-order convergence to the closed
form, the six face axes); and every injected defect rejected, so the assertions are shown to bite.  `-s` prints the measured figures."""
import numpy as np
import pytest

import sh9_truth as st
from direct12pbrrenderer_amd.scene import sh_pack_struct

CPU_SIZES = (1, 2, 3, 7, 64, 85, 86, 257, 300)
AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]   # D3D cube faces +x -x +y -y +z -z, written out


def orc_pack(orc, sky, size):
    return orc.sh9_project(np.ascontiguousarray(sky).reshape(-1), size)


def test_bands_are_the_derived_ones():
    assert np.allclose(st.KAPPA_TERM, [28.5, 39.8, 55.0], atol=0.06)
    assert np.allclose(st.LAMBERT, [1, 2 / 3, 1 / 4], rtol=2e-7, atol=0)               # K_l A_l / pi
    rows = {1: 1, 85: 1, 86: 2, 255: 4, 256: 4, 257: 8, 300: 8, 512: 16, 1024: 64, 1025: 64, 2048: 256, 8192: 4096}
    assert {s: st.launch_rows(s) for s in rows} == rows
    assert st.launch_blocks(85) == 510 and st.launch_blocks(1025) == 510 and st.launch_blocks(512) == 384
    assert all(st.launch_blocks(s) <= 512 for s in range(1, 2100)) and st.launch_blocks(8192) <= 512
    assert st.kappa_acc(512) == 24 and st.kappa_acc(8192) == 4104
    # the rounded constants are the rule: int Y_n^2 differs from 1 by a few 1e-6, which the closed form carries
    assert 1e-7 < np.abs((st.BASIS / st.EXACT) ** 2 - 1).max() < 5e-6


@pytest.mark.parametrize("kind", list(st.SKIES))
@pytest.mark.parametrize("size", CPU_SIZES)
def test_oracle_projection_in_band(orc, kind, size):
    sky, truth = st.sky_case(kind, size)
    assert np.isnan(sky[:, 3]).all()
    worst = st.check_pack(orc_pack(orc, sky, size), truth, 0, f"oracle {kind} {size}")
    print(f"oracle {kind} {size}: worst {worst:.2f} units of u S Ymax GAIN (kappa_term {st.KAPPA_TERM.tolist()})")


@pytest.mark.parametrize("face", range(6))
def test_one_hot_faces(orc, face):
    """the truth alone: the linear part of a one-face sky points along that face's axis (the axes written out above, not taken from
    the truth's table); then the oracle under the same assertion"""
    size = 7
    pack, S = st.project(st.one_hot_sky(size, face), size)
    lin = pack[0:3]
    assert np.allclose(lin / np.linalg.norm(lin), AXES[face], atol=1e-12)
    assert np.allclose(pack[8:11], 0.5 * lin, rtol=1e-12, atol=1e-15) and np.allclose(pack[16:19], 0.25 * lin, rtol=1e-12, atol=1e-15)
    assert np.array_equal(st.FACE_AXIS[face], AXES[face])
    st.check_one_hot(orc_pack(orc, st.one_hot_sky(size, face), size), size, face, 0, "oracle")


def test_second_order_convergence_to_the_closed_form():
    a = st.band_coefficients()
    want = st.closed_form(a)
    err = [np.abs(st.sky_case("band", s)[1][0] - want).max() for s in (16, 32, 64, 128, 256)]
    ratios = [err[i] / err[i + 1] for i in range(4)]
    print(f"|project - closed_form|: {['%.3e' % e for e in err]}, ratios {['%.3f' % r for r in ratios]}")
    assert all(r >= 3.5 for r in ratios)
    # the limit irradiance written from the expansion equals the closed form's pack evaluated: Q16's + c6 included
    pts = st.sphere_points()
    assert np.abs(st.irradiance(want, pts) - st.closed_form_irradiance(a, pts)).max() < 1e-14
    plain = np.moveaxis(np.tensordot(st.LAMBERT[st.BAND_OF] * a * (st.BASIS / st.EXACT) ** 2, st.basis(pts), axes=(1, 0)), 0, -1)
    c6 = st.closed_form(a)[[6, 14, 22]] / 3
    assert np.abs(st.irradiance(want, pts) - (plain + c6)).max() < 1e-14


def test_oracle_env_diffuse_in_band(orc):
    """orc.env_diffuse on the every-normal frame's pixels (every 5th column: all five metallic bytes, 13 k pixels), given the fp32
    normal, albedo and metallic: the truth is evaluated at those numbers, so the normal's own band is zero"""
    pack = np.float32(st.sky_case("band", 64)[1][0])
    sh = sh_pack_struct(pack)
    _, _, _, alb, metal = st.normal_frame()
    y, x = np.mgrid[0:256, 0:256]
    n64, _ = st.octa_decode(x, y)
    sel = (slice(None), slice(0, 256, 5))
    n32, a32, m32 = np.float32(n64[sel]).reshape(-1, 3), np.float32(alb[sel] / 255.0).reshape(-1, 3), np.float32(metal[sel] / 255.0).reshape(-1)
    got = np.array([orc.env_diffuse(sh, a32[i], float(m32[i]), n32[i]) for i in range(len(m32))])
    truth = st.evaluate_f(pack.astype(np.float64), n32.astype(np.float64), a32.astype(np.float64), m32.astype(np.float64))
    band = st.eval_band_f(pack.astype(np.float64), n32.astype(np.float64), 0.0, a32.astype(np.float64), m32.astype(np.float64))
    worst = st.check_eval(got, truth, band, "orc.env_diffuse")
    assert np.all(got[m32 == 1.0] == 0.0)
    print(f"orc.env_diffuse: worst {worst:.3f} of the band over {got.size} values")


def test_half_ties_stay_under_the_cap():
    """the truth alone: on the every-normal frame with the fp32 pack of the band sky at 256, the share of values whose band reaches a
    rounding tie of the half format is under the cap the GPU test asserts; metallic byte 255 is exactly 0 with a zero band"""
    pack = np.float32(st.sky_case("band", 256)[1][0]).astype(np.float64)
    truth, band = st.frame_truth(pack)
    _, decided = st.half_decided(truth, band)
    metal = st.normal_frame()[4]
    share = 1.0 - decided.mean()
    rel = band[truth != 0] / np.abs(truth[truth != 0])
    print(f"half ties: {share:.4%} undecided (cap {st.TIE_CAP:.1%}); band / |truth|: median {np.median(rel) / st.U:.1f} u, max {rel.max() / st.U:.1f} u")
    assert share <= st.TIE_CAP
    assert np.all(truth[metal == 255] == 0) and np.all(band[metal == 255] == 0) and decided[metal == 255].all()
    assert st.irradiance(pack, st.sphere_points()).min() > 0.1           # the band sky's irradiance keeps away from zero


# ------------------------------------------------------------------------------------------------------ the checks bite
def _cube(sky, size):
    return np.array(sky).reshape(6, size, size, 4)


def drop_column(sky, size):
    c = _cube(sky, size)
    c[:, :, size - 1, :3] = 0                                  # the second column block's one live lane at 257
    return c.reshape(-1, 4)


def double_last_rows(sky, size):
    c = _cube(sky, size)
    first = (size // st.launch_rows(size)) * st.launch_rows(size)
    assert 0 < size - first < st.launch_rows(size)
    c[:, first:, :, :3] *= 2                                   # the projection is linear: counting the ragged block twice
    return c.reshape(-1, 4)


def negate_u_face5(sky, size):
    c = _cube(sky, size)
    c[5] = c[5, :, ::-1].copy()
    return c.reshape(-1, 4)


def swap_g_b(sky, size):
    c = _cube(sky, size)
    c[..., [1, 2]] = c[..., [2, 1]]
    return c.reshape(-1, 4)


SKY_DEFECTS = {"column dropped at 257": (257, drop_column), "last row block twice at 300": (300, double_last_rows),
               "u negated on face 5": (64, negate_u_face5), "g and b swapped": (64, swap_g_b)}


@pytest.mark.parametrize("name", list(SKY_DEFECTS))
def test_defect_in_the_sky_is_rejected(orc, name):
    size, defect = SKY_DEFECTS[name]
    sky, truth = st.sky_case("band", size)
    st.check_pack(orc_pack(orc, sky, size), truth, 0, "control")
    with pytest.raises(AssertionError):
        st.check_pack(orc_pack(orc, defect(sky, size), size), truth, 0, name)


def swap_basis(p):
    for ch in range(3):
        p[8 * ch + 4], p[8 * ch + 5] = p[8 * ch + 5], p[8 * ch + 4]          # c4 <-> c5


def swap_w(p):
    for ch in range(3):
        p[8 * ch + 3], p[8 * ch + 7] = p[8 * ch + 7], p[8 * ch + 3]          # sha.w <-> shb.w


def restore_c6(p):
    for ch in range(3):
        p[8 * ch + 3] -= p[8 * ch + 6] / 3                                   # sha.w = c0 - c6: what Q16 drops


@pytest.mark.parametrize("defect", [swap_basis, swap_w, restore_c6])
def test_defect_in_the_pack_is_rejected(defect):
    pack, S = st.sky_case("band", 64)[1]
    bad = pack.copy()
    defect(bad)
    st.check_pack(pack.copy(), (pack, S), 0, "control")
    with pytest.raises(AssertionError):
        st.check_pack(bad, (pack, S), 0, defect.__name__)


def test_small_coefficient_is_held_to_its_own_scale():
    """a channel 1000 x darker than the others: 2^-18 of its DC coefficient is rejected, though it is 4e-9 of the pack's maximum and
    the 1e-5 max|pack| rule of test_sh9_vs_oracle lets it pass"""
    size = 64
    sky = np.array(st.sky_case("hdr", size)[0])
    sky[:, 2] *= np.float32(1e-3)
    pack, S = st.project(sky, size)
    i = 16 + 3                                                                 # sha_b.w = c0 of blue
    assert 3e-4 < abs(pack[i]) / np.abs(pack).max() < 3e-3
    bad = pack.copy()
    bad[i] *= 1 + 2.0 ** -18
    assert np.abs(bad - pack).max() <= 1e-5 * np.abs(pack).max()
    with pytest.raises(AssertionError):
        st.check_pack(bad, (pack, S), 0, "2^-18 of a small coefficient")
    bad[i] = pack[i] * (1 + 2.0 ** -21)                                         # 8 u: inside any band of an fp32 sum
    st.check_pack(bad, (pack, S), 0, "control")
