"""Float64 truth for the diffuse half of the image-based lighting: the SH9 projection of a sky cube's level 0 (SH.cpp:6-37, :98-151,
:201-222 as the deterministic texel quadrature of oracle/pbr_oracle.cpp) and its evaluation at a pixel's normal
(deferred_shading.hlsl:23-54), restated in plain numpy from the formulas, with the bands inside which an fp32 implementation may
differ from it, the skies the CPU and GPU tests share, and the assertions both run.  No GPU, no oracle and no project code in here:
tests/test_sh9_truth_cpu.py holds the CPU oracle to these assertions, tests/test_gpu_sh9_truth.py the kernels.

The rule.  Texel (x, y) of face f of a size^2 cube has the centre u = 2 (x + 1/2) / size - 1, v likewise, the raw direction
FACE_RAW[f] . (u, v, 1), d = raw / |raw| and the solid angle dw = (4 / size^2) / |raw|^3.  L[ch, n] = sum colour[ch] Y_n(d) dw over
the 6 size^2 texels, Y_n the nine real SH basis functions with the reference's six-digit constants (the fp32 literals widened: the
rounded constants ARE the rule).  c[ch, n] = INV_PI K_l A_l L[ch, n] basis_n with pi the fp32 value (quirk Q17: 1 / pi enters here
and again in the evaluation), then the pack: sha = (c3, c1, c2, c0), shb = (c4, c5, 3 c6, c7) (quirk Q16: the -c6 of c6 (3 z^2 - 1) is
dropped), shc = (c8 r, c8 g, c8 b, 0).  The evaluation: irradiance = sha . (n, 1) + shb . (xy, yz, zz, zx) + shc (xx - yy), times
albedo (1 - metallic) INV_PI with the bytes divided by 255.

The bands are derived from the number formats, not tuned.  u = 2^-24 is fp32's unit roundoff (one rounding is a relative error <= u,
one ULP is 2u).  v_rsq_f32 is taken as 1 ULP (AMD "CDNA3 / CDNA4 Instruction Set Architecture", VOP1 opcode table: V_RSQ_F32, "1ULP
accuracy"); 1.0f / x and sqrtf are correctly rounded in HIP's default mode and on the CPU.

PROJECTION.  |pack - truth| <= kappa u S_ch Ymax_n GAIN_n + FINISH u |c_n|, S_ch = sum |colour[ch]| dw (an ABSOLUTE sum: the terms
of a coefficient cancel, their roundings do not), Ymax_n = sup |Y_n| (not |Y_n|: 3 z^2 - 1 cancels inside a term), GAIN_n = |dc_n /
dL_n| of the pack slot (3 x for shb.z), kappa = kappa_term(l) + kappa_acc(size).
kappa_term(l) bounds the fp32 roundings of ONE term colour dw Y_n in units of u |colour| dw Ymax_n (kappa_term() evaluates it):
* the coordinates: inv_size = 1 / size (u), t = 2 (x + 1/2) inv_size (u) and t - 1 (u |u|): |delta u| <= (2 (1 + |u|) + |u|) u, the
  same for v.  The term depends on them through d (|grad Y_n| <= G_l Ymax_n on the sphere, G = 0, 1, 2, and |dd / du| <= 1 / |raw|) and
  through |raw|^-3 (relative 3 |u| / |raw|^2): sup over the face of sum_{w = u, v} (2 + 3 |w|) (G_l / |raw| + 3 |w| / |raw|^2) =
  10.0, 15.8, 21.5 for l = 0, 1, 2 (on a grid; met at the face's corner);
* |raw|^2 = 1 + u u + v v: two products and two sums of positive terms, 3u, halved by the root; v_rsq_f32 2u: inv = 1 / |raw| to
  3.5u.  It enters the term 3 + l times (d^l dw): (3 + l) 3.5u;
* d = raw inv, one rounding per component: l u through a homogeneous Y_n, 3u through 3 z^2 - 1 (6 z^2 u of 0.315392, against Ymax
  0.630784): 0, 1, 3;
* inv^3 two products (2u), dw0 = 4 inv_size inv_size (inv_size twice and a product: 3u), dw = dw0 inv^3 (u): 6u;
* Y_n itself: nothing for l = 0 (the literal), one product for l = 1, and for l = 2 at worst 3 dz, (3 dz) dz, - 1 (8u absolute of
  0.315392: 4u of Ymax) and the constant's product: 0, 1, 5;
* colour dw and its product with Y_n: 2u.
  kappa_term = 28.5, 39.8, 55.0 for l = 0, 1, 2.  A worst case: the errors of a sum of many terms do not line up, and both the
  oracle and the kernel measure a few units.
kappa_acc(size) is the kernel's fp32 accumulation: a thread adds launch_rows(size) terms into each accumulator (each addition rounds
to u of a partial sum that is at most the thread's absolute sum), the wave butterfly adds 6 levels, the four waves 2 more:
rows + 8.  The second stage sums the table in fp64 and contributes nothing at this scale.  The oracle accumulates in double:
kappa_acc = 0.  launch_rows() restates the launch rule of pbr_sh9_project.
FINISH = 12: K_l and A_l (a divide or product, a root that halves it and rounds: <= 3u each even with 1-ULP roots), and six more
roundings (INV_PI K, . A, the sum's conversion to fp32, . L, . basis_n, . 3).

EVALUATION.  Per pixel and channel, against evaluate() at the float64 octahedral decode of the pixel's bytes:
|out - truth| <= albedo (1 - metallic) INV_PI (E_n + u R) + KD_ROUNDINGS u |truth|: E_n and R are absolute scales of that pixel's
ten-term sum, whose terms cancel; at most R <= 12 sum |terms|.
* E_n = sum_j |d irradiance / d n_j| delta_n_j is the normal's own error: byte inv255 (inv255 and the product: 2u of the value),
  2 . - 1 (u of the result), d.z = 1 - |d.x| - |d.y| (two more roundings) or, folded, 1 - |d.y| (one more); normalised by
  the 1-ULP rsq of a three-product, two-sum dot (3.5u) and a product (u): delta_n = |I - n n^T| delta_d / |d| + 4.5 u |n|, per pixel;
* R counts the sum's own roundings in its association (_irradiance_parts): the products (one for a linear term, two for a quadratic
  one, four for shc's xx - yy), each u of its term, and the eight additions, each u of its own partial sum;
* KD_ROUNDINGS = 7: kd = (255 - metallic byte) k1, k1 = (inv255 inv255) INV_PI (inv255 twice, two products: 4u), the difference exact,
  its product u; kd albedo u; its product with the irradiance u.  The band is zero where the truth is (metallic byte 255).
The half target holds round_to_half(truth) wherever the truth is further than its band from a rounding tie (half_decided()).
"""
import functools

import numpy as np

U = 2.0 ** -24


def _f32(x):
    return float(np.float32(x))


PI = _f32(3.14159265359)
INV_PI = _f32(0.31830988618)
BASIS = np.array([_f32(c) for c in (0.282095, 0.488603, 0.488603, 0.488603, 1.092548, 1.092548, 0.315392, 1.092548, 0.546274)])
# the real orthonormal SH constants the six digits approximate: 1/2 sqrt(1/pi), sqrt(3/(4 pi)), 1/2 sqrt(15/pi), 1/4 sqrt(5/pi), 1/4 sqrt(15/pi)
EXACT = np.array([0.5 * np.sqrt(1 / np.pi)] + [np.sqrt(3 / (4 * np.pi))] * 3 + [0.5 * np.sqrt(15 / np.pi)] * 2
                 + [0.25 * np.sqrt(5 / np.pi), 0.5 * np.sqrt(15 / np.pi), 0.25 * np.sqrt(15 / np.pi)])
BAND_OF = np.array([0, 1, 1, 1, 2, 2, 2, 2, 2])
YMAX = BASIS * np.array([1, 1, 1, 1, 0.5, 0.5, 2, 0.5, 1])     # x y <= 1/2, |3 z^2 - 1| <= 2, |x^2 - y^2| <= 1
_K = np.sqrt(4 * PI / (2 * np.arange(3) + 1))                  # SH.cpp:140-151
_A = np.array([np.sqrt(PI) / 2, np.sqrt(PI / 3), np.sqrt(5 * PI) / 8])   # SH.cpp:70-85
LAMBERT = INV_PI * _K * _A                                     # 1, 2/3, 1/4 up to the fp32 pi
assert np.allclose(LAMBERT, [1, 2 / 3, 1 / 4], rtol=1e-6, atol=0)
GAIN = LAMBERT[BAND_OF] * BASIS                                # dc_n / dL_n
FINISH = 12
KD_ROUNDINGS = 7
TIE_CAP = 0.005                                                # share of the half target's values that may sit on a rounding tie

# cube_dir_raw: raw = FACE_RAW[f] @ (u, v, 1).  Faces +x, -x, +y, -y, +z, -z.
FACE_RAW = np.array([
    [[0, 0, 1], [0, -1, 0], [-1, 0, 0]],
    [[0, 0, -1], [0, -1, 0], [1, 0, 0]],
    [[1, 0, 0], [0, 0, 1], [0, 1, 0]],
    [[1, 0, 0], [0, 0, -1], [0, -1, 0]],
    [[1, 0, 0], [0, -1, 0], [0, 0, 1]],
    [[-1, 0, 0], [0, -1, 0], [0, 0, -1]],
], dtype=np.float64)
FACE_AXIS = FACE_RAW[:, :, 2]                                  # the direction of a face's centre


def basis(d):
    """the nine basis functions at unit directions d [..., 3] -> [9, ...] (SH.cpp:6-37: 1, y, z, x, xy, yz, 3zz - 1, xz, xx - yy)"""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    poly = [np.ones_like(x), y, z, x, x * y, y * z, 3 * z * z - 1, x * z, x * x - y * y]
    return np.stack([c * p for c, p in zip(BASIS, poly)])


def face_dirs(size, f):
    """(d [size, size, 3], dw [size, size]) of face f, rows y, columns x"""
    c = 2 * (np.arange(size, dtype=np.float64) + 0.5) / size - 1
    v, u = np.meshgrid(c, c, indexing="ij")
    raw = np.stack([u, v, np.ones_like(u)], axis=-1) @ FACE_RAW[f].T
    r2 = (raw * raw).sum(-1)
    return raw / np.sqrt(r2)[..., None], (4.0 / (size * size)) / (r2 * np.sqrt(r2))


def level0(sky, size):
    """the colour channels of level 0 of a cube [texels, 4] (or flat): [6, size, size, 3] float64; alpha and later mips are not read"""
    return np.asarray(sky).reshape(-1, 4)[:6 * size * size, :3].reshape(6, size, size, 3).astype(np.float64)


def moments(sky, size):
    """(L [3, 9], S [3]): L[ch, n] = sum colour Y_n dw, S[ch] = sum |colour| dw, face by face"""
    col = level0(sky, size)
    L, S = np.zeros((3, 9)), np.zeros(3)
    for f in range(6):
        d, dw = face_dirs(size, f)
        w = (basis(d) * dw).reshape(9, -1)
        c = col[f].reshape(-1, 3)
        L += (w @ c).T
        S += np.abs(c).T @ dw.reshape(-1)
    return L, S


def pack_of(c):
    """c [3, 9] -> the 28-float pack (SH.cpp:201-222)"""
    p = np.zeros(28)
    for ch in range(3):
        p[8 * ch:8 * ch + 4] = c[ch, 3], c[ch, 1], c[ch, 2], c[ch, 0]
        p[8 * ch + 4:8 * ch + 8] = c[ch, 4], c[ch, 5], 3 * c[ch, 6], c[ch, 7]
        p[24 + ch] = c[ch, 8]
    return p


# pack slot -> (channel, coefficient) and back, for messages and for the defects of the CPU tests
SLOT = {}
for _ch in range(3):
    for _k, _n in enumerate((3, 1, 2, 0, 4, 5, 6, 7)):
        SLOT[8 * _ch + _k] = (_ch, _n)
    SLOT[24 + _ch] = (_ch, 8)


def slot_name(i):
    if i == 27:
        return "shc.w"
    ch, n = SLOT[i]
    return f"c{n} of channel {'rgb'[ch]} ({'sha' if i % 8 < 4 and i < 24 else 'shb' if i < 24 else 'shc'}.{'xyzw'[i % 4 if i < 24 else i - 24]})"


def project(sky, size):
    """(pack [28] float64, S [3]) of a sky cube's level 0"""
    L, S = moments(sky, size)
    return pack_of(GAIN * L), S


def launch_rows(size):
    """rows per block of k_sh9_partial: the launch rule of pbr_sh9_project (the table holds 512 rows)"""
    cols = -(-size // 256)
    rows = 1
    while cols * -(-size // rows) * 6 > 512:
        rows *= 2
    return rows


def launch_blocks(size):
    return -(-size // 256) * -(-size // launch_rows(size)) * 6


def kappa_term(l):
    """the fp32 roundings of one term colour dw Y_n, in units of u |colour| dw Ymax_n (module docstring)"""
    g = (0.0, 1.0, 2.0)[l]
    w = np.linspace(0.0, 1.0, 257)
    uu, vv = np.meshgrid(w, w)
    r2 = 1 + uu * uu + vv * vv
    coord = ((2 + 3 * uu) * (g / np.sqrt(r2) + 3 * uu / r2) + (2 + 3 * vv) * (g / np.sqrt(r2) + 3 * vv / r2)).max()
    return coord + (3 + l) * 3.5 + (0, 1, 3)[l] + 6 + (0, 1, 5)[l] + 2


KAPPA_TERM = np.array([kappa_term(l) for l in range(3)])
assert np.all(KAPPA_TERM > 2.2) and np.allclose(KAPPA_TERM, [28.5, 39.8, 55.0], atol=0.06)


def kappa_acc(size):
    return launch_rows(size) + 6 + 2


def pack_band(truth_pack, S, k_acc):
    """the absolute band of every pack slot [28] (0 for shc.w, which is written as 0)"""
    band = np.zeros(28)
    for i, (ch, n) in SLOT.items():
        scale = 3.0 if i < 24 and i % 8 == 6 else 1.0
        band[i] = (KAPPA_TERM[BAND_OF[n]] + k_acc) * U * S[ch] * YMAX[n] * GAIN[n] * scale + FINISH * U * abs(truth_pack[i])
    return band


def pack_units(got, truth_pack, S):
    """|got - truth| per slot in units of u S_ch Ymax_n GAIN_n (the figure kappa bounds); 0 for shc.w"""
    out = np.zeros(28)
    for i, (ch, n) in SLOT.items():
        scale = 3.0 if i < 24 and i % 8 == 6 else 1.0
        den = U * S[ch] * YMAX[n] * GAIN[n] * scale
        out[i] = abs(float(got[i]) - truth_pack[i]) / den if den else 0.0
    return out


def check_pack(got, truth, k_acc, what=""):
    """got [28] within its band of truth = (pack, S).  Returns the worst distance in units of u S Ymax GAIN."""
    pack, S = truth
    got = np.asarray(got, dtype=np.float64).reshape(28)
    assert np.all(np.isfinite(got)), f"{what}: a non-finite coefficient: {got}"
    assert got[27] == 0.0, f"{what}: shc.w = {got[27]!r}"
    err, band = np.abs(got - pack), pack_band(pack, S, k_acc)
    bad = np.nonzero(err > band)[0]
    if bad.size:
        i = bad[np.argmax((err / np.maximum(band, 1e-300))[bad])]
        raise AssertionError(f"{what}: {slot_name(i)}: got {got[i]!r}, truth {pack[i]!r}, off by {err[i]:.3e} = {err[i] / band[i]:.2f} bands "
                             f"({pack_units(got, pack, S)[i]:.1f} units); {bad.size} slots outside")
    return float(pack_units(got, pack, S).max())


# ---------------------------------------------------------------------------------------------------------------- evaluation
def irradiance(pack, n):
    """[..., 3]: sha . (n, 1) + shb . (xy, yz, zz, zx) + shc (xx - yy) per channel at unit normals n [..., 3]"""
    out, _, _ = _irradiance_parts(np.asarray(pack, dtype=np.float64), np.asarray(n, dtype=np.float64))
    return out


def _irradiance_parts(pack, n):
    """(irradiance, R = the roundings of the ten-term sum in units of u, gradient with respect to n [..., 3 channels, 3 components]).
    R follows the sum's association, ((s0 + s1) + s2) + s3 for sha and for shb, then + shc (xx - yy), then the two halves: every
    product rounds to u of itself (a quadratic term's polynomial first: 2u; xx - yy: u (xx + yy) + u |xx - yy|, then shc's product)
    and every addition to u of its own result."""
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    one, zero = np.ones_like(x), np.zeros_like(x)
    polys = [x, y, z, one, x * y, y * z, z * z, z * x]
    prods = [1, 1, 1, 0, 2, 2, 2, 2]
    grads = [(one, zero, zero), (zero, one, zero), (zero, zero, one), (zero, zero, zero), (y, x, zero), (zero, z, y), (zero, zero, 2 * z), (z, zero, x)]
    cc = x * x - y * y
    irr, rnd, grad = [], [], []
    for ch in range(3):
        co = pack[8 * ch:8 * ch + 8]
        t = [c * p for c, p in zip(co, polys)]
        tc = pack[24 + ch] * cc
        r = sum(k * np.abs(v) for k, v in zip(prods, t)) + np.abs(pack[24 + ch]) * (x * x + y * y + np.abs(cc)) + np.abs(tc)
        a1 = t[0] + t[1]; a2 = a1 + t[2]; a3 = a2 + t[3]
        b1 = t[4] + t[5]; b2 = b1 + t[6]; b3 = b2 + t[7]; b4 = b3 + tc
        s = a3 + b4
        r = r + sum(np.abs(v) for v in (a1, a2, a3, b1, b2, b3, b4, s))
        g = [sum(c * gr[j] for c, gr in zip(co, grads)) + pack[24 + ch] * (2 * x, -2 * y, zero)[j] for j in range(3)]
        irr.append(s); rnd.append(r); grad.append(np.stack(g, axis=-1))
    return np.stack(irr, axis=-1), np.stack(rnd, axis=-1), np.stack(grad, axis=-2)


def evaluate_f(pack, n, albedo, metallic):
    """environment_diffuse in float64 for an albedo [..., 3] and a metallic [...] given as numbers: irradiance albedo (1 - metallic) INV_PI"""
    return irradiance(pack, n) * np.asarray(albedo, dtype=np.float64) * (1.0 - np.asarray(metallic, dtype=np.float64)[..., None]) * INV_PI


def evaluate(pack, n, albedo_bytes, metal_byte):
    """evaluate_f with the G-buffer's bytes divided by 255 in float64.  Exactly 0 at metallic byte 255."""
    return evaluate_f(pack, n, np.asarray(albedo_bytes, dtype=np.float64) / 255.0, np.asarray(metal_byte, dtype=np.float64) / 255.0)


def octa_decode(ub, vb):
    """the unit normal of the G-buffer bytes (global.hlsli:101-115, :135-138; sign(0) = +1) and the first-order fp32 error of its
    components (module docstring): (n [..., 3], delta_n [..., 3] in absolute terms)"""
    fu, fv = np.asarray(ub, dtype=np.float64) / 255.0, np.asarray(vb, dtype=np.float64) / 255.0
    dx, dy = 2 * fu - 1, 2 * fv - 1
    ex, ey = (4 * fu + np.abs(dx)) * U, (4 * fv + np.abs(dy)) * U
    dz = 1 - np.abs(dx) - np.abs(dy)
    ez = ex + ey + (np.abs(1 - np.abs(dx)) + np.abs(dz)) * U
    fold = dz < 0
    assert np.all(np.abs(dz) > 1e-3)                                # |2a - 255| + |2b - 255| is even: no byte pair sits on the fold
    sx, sy = np.where(dx >= 0, 1.0, -1.0), np.where(dy >= 0, 1.0, -1.0)
    nx, ny = np.where(fold, sx * (1 - np.abs(dy)), dx), np.where(fold, sy * (1 - np.abs(dx)), dy)
    enx, eny = np.where(fold, ey + np.abs(nx) * U, ex), np.where(fold, ex + np.abs(ny) * U, ey)
    d = np.stack([nx, ny, dz], axis=-1)
    length = np.sqrt((d * d).sum(-1))
    n = d / length[..., None]
    e = np.stack([enx, eny, ez], axis=-1) / length[..., None]
    proj = np.abs(np.eye(3) - n[..., :, None] * n[..., None, :])    # d n / d d = (I - n n^T) / |d|
    return n, (proj * e[..., None, :]).sum(-1) + 4.5 * U * np.abs(n)


def eval_band_f(pack, n, delta_n, albedo, metallic):
    """the absolute band of the shaded diffuse term per pixel and channel [..., 3] (module docstring); delta_n = 0 where the normal is given"""
    irr, rnd, grad = _irradiance_parts(np.asarray(pack, dtype=np.float64), np.asarray(n, dtype=np.float64))
    e_n = (np.abs(grad) * np.broadcast_to(np.asarray(delta_n, dtype=np.float64), np.shape(n))[..., None, :]).sum(-1)
    kda = np.asarray(albedo, dtype=np.float64) * (1.0 - np.asarray(metallic, dtype=np.float64)[..., None]) * INV_PI
    return kda * (e_n + U * rnd) + KD_ROUNDINGS * U * np.abs(kda * irr)


def eval_band(pack, n, delta_n, albedo_bytes, metal_byte):
    return eval_band_f(pack, n, delta_n, np.asarray(albedo_bytes, dtype=np.float64) / 255.0, np.asarray(metal_byte, dtype=np.float64) / 255.0)


def check_eval(got, truth, band, what=""):
    """got [..., 3] within band of truth.  Returns the worst |got - truth| / band over the values with a band."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - truth)
    bad = err > band
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} values outside the band; first at {i}: got {got[i]!r}, truth {truth[i]!r}, "
                             f"off by {err[i]:.3e}, band {band[i]:.3e}")
    live = band > 0
    return float((err[live] / band[live]).max()) if live.any() else 0.0


def half_decided(truth, band):
    """(round_to_half(truth), decided): decided where no rounding tie of the half format lies within the band of the truth, i.e.
    where truth - band and truth + band round to the same half"""
    with np.errstate(over="ignore"):
        lo, hi, mid = (np.asarray(v).astype(np.float16) for v in (truth - band, truth + band, truth))
    return mid, lo == hi


# ---------------------------------------------------------------------------------------------------------------- skies
NAN = np.float32(np.nan)


def _cube(colour):
    """[6, size, size, 3] float64 -> [6 size^2, 4] float32 with alpha = NaN (nothing may read it)"""
    sky = np.full(colour.shape[:3] + (4,), NAN, dtype=np.float32)
    with np.errstate(over="ignore"):
        sky[..., :3] = colour
    return sky.reshape(-1, 4)


def band_coefficients(seed=0x5B9):
    """a [3, 9]: coefficients in [-1, 1] with a DC term of 3, a different vector per channel (a channel swap shows)"""
    a = np.random.default_rng(seed).uniform(-1.0, 1.0, (3, 9))
    a[:, 0] = 3.0
    return a


def band_sky(size, a=None):
    """L(d) = sum a[ch, n] Y_n(d) at the texel centres"""
    a = band_coefficients() if a is None else a
    return _cube(np.stack([np.moveaxis(np.tensordot(a, basis(face_dirs(size, f)[0]), axes=(1, 0)), 0, -1) for f in range(6)]))


def hdr_sky(size):
    """log-uniform 2^-10 .. 2^4 with one 5e4 sun texel off-centre on face 2"""
    rng = np.random.default_rng(0x4D52 + size)
    col = np.exp2(rng.uniform(-10.0, 4.0, (6, size, size, 3)))
    col[2, (2 * size) // 3, size // 4] = 5e4
    return _cube(col)


def signed_sky(size):
    return _cube(np.random.default_rng(0x519 + size).standard_normal((6, size, size, 3)))


def one_hot_sky(size, face):
    col = np.zeros((6, size, size, 3))
    col[face] = (1.0, 0.5, 0.25)
    return _cube(col)


SKIES = {"band": band_sky, "hdr": hdr_sky, "signed": signed_sky}


@functools.lru_cache(maxsize=None)
def sky_case(kind, size):
    """(sky, (pack, S)) of SKIES[kind] at size, computed once per process and shared: treat both as read-only"""
    sky = SKIES[kind](size)
    sky.setflags(write=False)
    return sky, project(sky, size)


def check_one_hot(got, size, face, k_acc, what=""):
    """the linear part sha.xyz of a sky with only `face` lit points along that face's axis, with its sign: the on-axis component is
    the truth's within the band and at least 1000 bands from 0, the two others are 0 within theirs"""
    truth = project(one_hot_sky(size, face), size)
    band = pack_band(*truth, k_acc)
    got = np.asarray(got, dtype=np.float64)
    for ch in range(3):
        lin = got[8 * ch:8 * ch + 3]
        for j in range(3):
            i = 8 * ch + j
            if FACE_AXIS[face, j] != 0:
                assert lin[j] * FACE_AXIS[face, j] > 1000 * band[i], f"{what} face {face}: {slot_name(i)} = {lin[j]!r} does not point along the face's axis"
            else:
                assert abs(lin[j]) <= band[i], f"{what} face {face}: {slot_name(i)} = {lin[j]!r}, off the axis"
    return check_pack(got, truth, k_acc, f"{what} one-hot face {face}")


# ---------------------------------------------------------------------------------------------------------------- closed form
def closed_form(a):
    """the continuous limit of the pack of band_sky(., a): the rounded basis functions are multiples of an orthonormal set, so
    L[ch, n] -> a[ch, n] int Y_n^2 = a[ch, n] (basis_n / exact_n)^2 (without the squared ratio the limit sits 4e-6 off)"""
    return pack_of(GAIN * np.asarray(a, dtype=np.float64) * (BASIS / EXACT) ** 2)


def closed_form_irradiance(a, n):
    """the limit irradiance written from the expansion, not through the pack: sum_n (A_l / pi) a_n int Y_n^2 Y_n(n) + c6 (Q16's
    dropped constant)"""
    c = GAIN * np.asarray(a, dtype=np.float64) * (BASIS / EXACT) ** 2                     # [3, 9]
    poly = basis(np.asarray(n, dtype=np.float64)) / BASIS.reshape((9,) + (1,) * (np.ndim(n) - 1))
    return np.moveaxis(np.tensordot(c, poly, axes=(1, 0)), 0, -1) + c[:, 6]


def sphere_points(k=64):
    """unit vectors on a latitude / longitude grid, poles included"""
    t, p = np.meshgrid(np.linspace(0, np.pi, k), np.linspace(0, 2 * np.pi, 2 * k, endpoint=False), indexing="ij")
    return np.stack([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)], axis=-1)


# ---------------------------------------------------------------------------------------------------------------- the every-normal frame
METAL_CYCLE = (0, 1, 128, 254, 255)


def normal_frame():
    """the 256 x 256 G-buffer tile whose plane B holds every (u, v) byte pair once: planes A, B, C (uint32), the albedo bytes
    [256, 256, 3] and the metallic byte [256, 256].  Albedo varies along x (three different ramps), the metallic byte cycles by row
    through METAL_CYCLE, the roughness varies, emission 0."""
    y, x = np.mgrid[0:256, 0:256].astype(np.uint32)
    alb = np.stack([x, (x * 7 + 13) & 255, 255 - x], axis=-1)
    metal = np.array(METAL_CYCLE, dtype=np.uint32)[y % 5]
    rough = (x * 5 + y * 3) & 255
    A = alb[..., 0] | (alb[..., 1] << 8) | (alb[..., 2] << 16)
    B = x | (y << 8) | np.uint32(0x00FF0000)
    Cc = rough | (metal << 8) | (np.uint32(0x80) << 16)
    return A.astype(np.uint32), B.astype(np.uint32), Cc.astype(np.uint32), alb.astype(np.int64), metal.astype(np.int64)


def frame_truth(pack):
    """(truth [256, 256, 3], band) of the every-normal frame shaded with `pack` alone (no lights, black specular)"""
    _, _, _, alb, metal = normal_frame()
    y, x = np.mgrid[0:256, 0:256]
    n, dn = octa_decode(x, y)
    return evaluate(pack, n, alb, metal), eval_band(pack, n, dn, alb, metal)
