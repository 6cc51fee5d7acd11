"""The sky resolve (include/pbr_hip.h: pbr_skybox; DESIGN.md, "Sky resolve under float64 truth") in plain numpy float64, and the one
check that holds an image to it.  Written from the pass's definition, not from the fp32 code: it imports no project code and shares no
arithmetic with oracle/pbr_oracle.cpp or csrc/raster.hip.

THE PASS.  For every pixel of a tile whose stencil is 0:
  ray      d = InvView3x3 . (ndc_x near_width / 2, ndc_y near_height / 2, Near), ndc of the pixel centre (y up), near_height =
           2 Near tan(Fov / 2), near_width = near_height Ratio.
  face     the largest |component| of d (ties: x before y before z); (u, v) = (sc, tc) / ma in [-1, 1], faces +x -x +y -y +z -z with
           (sc, tc) = (-z, -y) (z, -y) (x, z) (x, -z) (x, -y) (-x, -y).
  LOD      the rays through (x + 1, y) and (x, y + 1) projected onto the CENTRE pixel's face; rho = size / 2 . max(|D_x|, |D_y|), D the
           difference of face coordinates as a 2-vector; lod = log2(rho) clamped to [0, mips - 1] and snapped to 1 / 256 (round half up).
  levels   l0 = floor(lod), l1 = min(l0 + 1, mips - 1), weight f = lod - l0.  On a level of edge s the coordinate c = (u + 1) / 2 . s is
           clamped to [-1.5, s + 1.5], snapped to 1 / 256 (round half up) and moved by -0.5; its floor is the first tap, its fraction the
           weight (a multiple of 1 / 256).  A tap outside the face is replaced by the texel that the direction of ITS texel centre lands
           in (face rule above, floor, clamped to the face); a tap outside in both axes is first clamped in y.  A tap of weight exactly 0
           does not contribute.  x-lerps, then the y-lerp, then the level lerp; alpha 1; the result is rounded to half.

INTERVALS.  Three decisions can fall either way under rounding; the truth takes the union of what each alternative gives:
  face     a second axis within FACE_TIE_REL = 1e-6 (relative) of the largest one (oracle/pbr_oracle_f64.cpp, trilinear_interval).
  x.8 snap c . 256 + 0.5 within SNAP_TOL_ULPS = 16 . 2^-24 . max(|c| . 256, 1) of an integer (oracle/pbr_oracle_f64.cpp, snap_set).
  LOD snap lod . 256 + 0.5 within 256 T of an integer, T the forward error bound of the fp32 LOD, in LOD units, below.

T, THE FP32 LOD'S FORWARD ERROR (eps = 2^-24; |.| of the exact quantities).  The fp32 pass forms
  u_p = fl((gx + .5) / W), ndc = fl(2 u_p - 1): the division rounds once, the subtraction is exact for u_p >= 1/4 (Sterbenz) and
        rounds a value <= 1 otherwise: |d ndc| <= 2 eps.  cx = fl(ndc/2 . nw): |d cx| <= eps (2 hw + |cx|), hw = nw / 2; cy alike.
  d_i = fl(fl(fl(M_i0 cx) + fl(M_i1 cy)) + fl(M_i2 Near)): three products, two sums:
        e_i = eps [ |M_i0| (2 hw + 2 |cx|) + |M_i1| (2 hh + 2 |cy|) + |M_i2| Near + |M_i0 cx + M_i1 cy| + |d_i| ].
  u   = fl(sc / ma): |d u| <= (e_sc + |u| e_ma) / |ma| + eps |u|      — about eps (1 + |u|) times a small constant.
  D_u = fl(u_x - u_0): |d D_u| <= d u_x + d u_0 + eps |D_u|            — THE CANCELLATION: absolute errors of size eps (1 + |u|)
        on a difference of size |D_u|, a relative error of eps (1 + |u|) / |D_u| that grows as the frame gets wider in pixels.
  r   = fl(size/2 . sqrt(D_u^2 + D_v^2)): first order (|D_u| d D_u + |D_v| d D_v) / r^2 relative, plus 4 eps for the squares, the sum,
        the root and the product, plus 12 eps for near_width and near_height themselves (tanf to 1 ulp and two products: a common
        scale of cx and cy, which moves D by at most 3 times its relative size).
  lod = log2f(max(r_x, r_y)): the relative error of r over ln 2, plus log2f's own ulp, 2 eps (|lod| + 1).
  T   = max over the two neighbours of [ (|D_u| d D_u + |D_v| d D_v) / |D|^2 + 16 eps ] / ln 2 + 2 eps (|lod| + 1).
The clamp to [0, mips - 1] is monotone and 1-Lipschitz, so T holds for the clamped LOD too.  lod_f32() restates the fp32 formula for
ONE purpose: measuring its distance to the float64 LOD in units of T (tests/test_sky_truth_cpu.py prints the table).

THE CHECK (check()).  For stencil-0 pixels with flag 0, per channel: dist(got, [lo, hi]) <= E + S.
  S = 2^-11 |got| + 2^-25: round-to-nearest of the half store and half a subnormal step (as tests/shade_checks.py).
  E = E_ROUNDINGS . 2^-24 . M, M the largest |tap| of the pixel's eight taps.  The sample is seven lerps, r = fma(b, w, fl(a (1 - w))):
      1 - w is exact (w is a multiple of 1 / 256 in [0, 1)), the product rounds once, the fma once: at most 2 roundings, each of a
      value <= M since every intermediate is a convex combination of taps; 3 allows for a lerp written a + (b - a) w.  A lerp passes
      the errors of its inputs on with the same convex weights, so errors add along the DEPTH of the tree (x-lerp, y-lerp, level lerp:
      3), not over its seven nodes: E_ROUNDINGS = 3 . 3 = 9.
FLAGS (no single truth; capped by the tests): 1 a non-finite tap; 2 rho == 0 or not finite; 4 a face tie whose alternatives span more
than E beyond the widest of them.

truth(..., mutation=NAME) makes one deliberate mistake (MUTATIONS); the CPU tests show that check() rejects each."""
import math

import numpy as np

f64 = np.float64
EPS = 2.0 ** -24
FACE_TIE_REL = 1e-6
SNAP_TOL_ULPS = 16.0
E_ROUNDINGS = 9.0
FLAG_TAP, FLAG_RHO, FLAG_TIE = 1, 2, 4
MUTATIONS = ("lod_bias", "lod_x_only", "clamp_to_edge", "corner_x_first", "swap_faces_2_3", "no_snap")

# per face: (axis, sign) of ma, sc, tc
_MA = ((0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1))
_SC = ((2, -1), (2, 1), (0, 1), (0, 1), (0, 1), (0, -1))
_TC = ((1, -1), (1, -1), (2, 1), (2, -1), (1, -1), (1, -1))
_AX = {k: (np.array([t[f][0] for f in range(6)]), np.array([float(t[f][1]) for f in range(6)])) for k, t in (("ma", _MA), ("sc", _SC), ("tc", _TC))}


def camera_of(g):
    """the fields of a pbr_global the pass reads, from any object that has them, as float64 of their float32 values"""
    near, fov, ratio = float(np.float32(g.Near)), float(np.float32(g.Fov)), float(np.float32(g.Ratio))
    hh = near * math.tan(fov / 2.0)
    return {"M": np.array(g.InvView[:], dtype=np.float32).astype(f64).reshape(4, 4)[:3, :3], "Near": near, "Fov": fov, "Ratio": ratio,
            "hh": hh, "hw": hh * ratio}


def chain_texels(size, mips):
    return sum(6 * (size >> l) ** 2 for l in range(mips))


def levels_of(cube, size, mips):
    """a cube chain in the pbr_cube_f32 layout (levels concatenated, six faces per level, rows of RGBA) -> [6, s, s, 3] float64 per level"""
    cube = np.asarray(cube).reshape(-1, 4)
    assert cube.shape[0] == chain_texels(size, mips), (cube.shape, size, mips)
    out, o = [], 0
    for l in range(mips):
        s = size >> l
        out.append(cube[o:o + 6 * s * s, :3].astype(f64).reshape(6, s, s, 3))
        o += 6 * s * s
    return out


def _pick(d, face, which):
    axis, sign = _AX[which]
    return np.take_along_axis(d, axis[face][:, None], 1)[:, 0] * sign[face].astype(d.dtype)


def _project(d, face):
    ma = _pick(d, face, "ma")
    with np.errstate(divide="ignore", invalid="ignore"):
        return _pick(d, face, "sc") / ma, _pick(d, face, "tc") / ma, ma


def _major(a):
    """axis of the largest |component|, ties x before y before z"""
    return np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))


def _dir_raw(face, u, v):
    one = np.ones_like(u)
    return np.stack([np.choose(face, [one, -one, u, u, u, -u]), np.choose(face, [-v, -v, one, -one, -v, -v]),
                     np.choose(face, [-u, u, v, -v, one, -one])], axis=-1)


def _rays(cam, tile, gx, gy):
    """(direction [n, 3], its fp32 component error bound e [n, 3]) of the rays through the centres of global pixels (gx, gy)"""
    M, hw, hh, near = cam["M"], cam["hw"], cam["hh"], cam["Near"]
    cx = (2.0 * (gx + 0.5) / tile.full_w - 1.0) * hw
    cy = (1.0 - 2.0 * (gy + 0.5) / tile.full_h) * hh
    d = np.stack([M[i, 0] * cx + M[i, 1] * cy + M[i, 2] * near for i in range(3)], axis=-1)
    e = np.stack([abs(M[i, 0]) * (2.0 * hw + 2.0 * np.abs(cx)) + abs(M[i, 1]) * (2.0 * hh + 2.0 * np.abs(cy)) + abs(M[i, 2]) * near
                  + np.abs(M[i, 0] * cx + M[i, 1] * cy) + np.abs(d[:, i]) for i in range(3)], axis=-1) * EPS
    return d, e


def _coord_error(e, face, u, v, ma):
    e_ma, e_sc, e_tc = (np.take_along_axis(e, _AX[k][0][face][:, None], 1)[:, 0] for k in ("ma", "sc", "tc"))
    return (e_sc + np.abs(u) * e_ma) / np.abs(ma) + EPS * np.abs(u), (e_tc + np.abs(v) * e_ma) / np.abs(ma) + EPS * np.abs(v)


# ---- one level -------------------------------------------------------------------------------------------------------------------
def _fetch(level, s, face, x, y, mutation):
    """texels [n, 3] of the taps (face, x, y) under the seamless rule, and whether each tap left the face (in any axis, in both)"""
    xo, yo = (x < 0) | (x >= s), (y < 0) | (y >= s)
    out, both = xo | yo, xo & yo
    if mutation == "clamp_to_edge":
        f2, x2, y2 = face, np.clip(x, 0, s - 1), np.clip(y, 0, s - 1)
    else:
        if mutation == "corner_x_first":
            x = np.where(both, np.clip(x, 0, s - 1), x)
        else:
            y = np.where(both, np.clip(y, 0, s - 1), y)
        d = _dir_raw(face, 2.0 * (x + 0.5) / s - 1.0, 2.0 * (y + 0.5) / s - 1.0)
        ax = _major(np.abs(d))
        f2 = 2 * ax + (np.take_along_axis(d, ax[:, None], 1)[:, 0] < 0)
        u2, v2, _ = _project(d, f2)
        x2 = np.clip(np.floor((u2 + 1.0) * 0.5 * s), 0, s - 1).astype(np.int64)
        y2 = np.clip(np.floor((v2 + 1.0) * 0.5 * s), 0, s - 1).astype(np.int64)
    f, xx, yy = np.where(out, f2, face), np.where(out, x2, x), np.where(out, y2, y)
    if mutation == "swap_faces_2_3":
        f = np.where(f == 2, 3, np.where(f == 3, 2, f))
    return level[f, yy, xx], out, both


def _bilinear(level, s, face, X, Y, mutation):
    """the footprint at the snapped positions (X, Y) (texel units, half-texel offset removed): value [n, 3], largest |tap|, any
    non-finite tap, any tap off the face, any tap off it in both axes"""
    fx, fy = np.floor(X), np.floor(Y)
    x0, y0, wx, wy = fx.astype(np.int64), fy.astype(np.int64), (X - fx)[:, None], (Y - fy)[:, None]
    taps = [_fetch(level, s, face, x0 + i, y0 + j, mutation) for j in (0, 1) for i in (0, 1)]
    with np.errstate(invalid="ignore", over="ignore"):
        lerp = lambda a, b, w: np.where(w == 0.0, a, a * (1.0 - w) + b * w)
        val = lerp(lerp(taps[0][0], taps[1][0], wx), lerp(taps[2][0], taps[3][0], wx), wy)
    mag = np.max([np.abs(t[0]).max(axis=-1) for t in taps], axis=0)
    bad = np.any([~np.isfinite(t[0]).all(axis=-1) for t in taps], axis=0)
    return val, mag, bad, np.any([t[1] for t in taps], axis=0), np.any([t[2] for t in taps], axis=0)


def _snaps(c, s, mutation):
    """(the exact snapped position, the other one an fp32 evaluation can land on — the same where there is none)"""
    c = np.clip(c, -1.5, s + 1.5)
    if mutation == "no_snap":
        return c - 0.5, c - 0.5
    t = c * 256.0 + 0.5
    fl = np.floor(t)
    tol = SNAP_TOL_ULPS * EPS * np.maximum(np.abs(c) * 256.0, 1.0)
    other = np.where(t - fl < tol, fl - 1.0, np.where(fl + 1.0 - t < tol, fl + 1.0, fl))
    return fl / 256.0 - 0.5, other / 256.0 - 0.5


def _level_interval(level, s, face, U, V, mutation):
    xm, xa = _snaps(U * s, s, mutation)
    ym, ya = _snaps(V * s, s, mutation)
    val, mag, bad, edge, corner = _bilinear(level, s, face, xm, ym, mutation)
    lo, hi = val.copy(), val.copy()
    wide = (xa != xm) | (ya != ym)
    k = np.flatnonzero(wide)
    if len(k):
        for X, Y in ((xa, ym), (xm, ya), (xa, ya)):
            v2, m2, b2, _, _ = _bilinear(level, s, face[k], X[k], Y[k], mutation)
            lo[k], hi[k], mag[k], bad[k] = np.fmin(lo[k], v2), np.fmax(hi[k], v2), np.maximum(mag[k], m2), bad[k] | b2
    return lo, hi, mag, bad, wide, edge, corner


def _levels_interval(levels, size, face, U, V, l, mutation):
    n = len(face)
    lo, hi, mag = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    bad, wide, edge, corner = (np.zeros(n, bool) for _ in range(4))
    for ll in np.unique(l):
        k = np.flatnonzero(l == ll)
        lo[k], hi[k], mag[k], bad[k], wide[k], edge[k], corner[k] = _level_interval(levels[ll], size >> int(ll), face[k], U[k], V[k], mutation)
    return lo, hi, mag, bad, wide, edge, corner


def _trilinear(levels, size, mips, face, U, V, lod_s, mutation):
    l0 = np.floor(lod_s).astype(np.int64)
    l1 = np.minimum(l0 + 1, mips - 1)
    f = (lod_s - l0)[:, None]
    lo, hi, mag, bad, wide, edge, corner = _levels_interval(levels, size, face, U, V, l0, mutation)
    k = np.flatnonzero((f[:, 0] != 0.0) & (l1 != l0))
    if len(k):
        lo1, hi1, m1, b1, w1, e1, c1 = _levels_interval(levels, size, face[k], U[k], V[k], l1[k], mutation)
        with np.errstate(invalid="ignore", over="ignore"):
            lo[k], hi[k] = lo[k] * (1.0 - f[k]) + lo1 * f[k], hi[k] * (1.0 - f[k]) + hi1 * f[k]
        mag[k], bad[k], wide[k], edge[k], corner[k] = np.maximum(mag[k], m1), bad[k] | b1, wide[k] | w1, edge[k] | e1, corner[k] | c1
    return lo, hi, mag, bad, wide, edge, corner


# ---- one candidate face ----------------------------------------------------------------------------------------------------------
def _footprint(size, face, rays, mutation):
    """(u, v in [-1, 1], raw lod, T, rho unusable) of the centre rays on `face`; rays = ((d, e) centre, x-neighbour, y-neighbour)"""
    (d0, e0), (dx, ex), (dy, ey) = rays
    u0, v0, m0 = _project(d0, face)
    du0, dv0 = _coord_error(e0, face, u0, v0, m0)
    rho, rel = [], []
    for d, e in ((dx, ex), (dy, ey)):
        u, v, m = _project(d, face)
        du, dv = _coord_error(e, face, u, v, m)
        Du, Dv = u - u0, v - v0
        r2 = Du * Du + Dv * Dv
        with np.errstate(divide="ignore", invalid="ignore"):
            rel.append((np.abs(Du) * (du + du0 + EPS * np.abs(Du)) + np.abs(Dv) * (dv + dv0 + EPS * np.abs(Dv))) / r2 + 16.0 * EPS)
        rho.append(0.5 * size * np.sqrt(r2))
    r = rho[0] if mutation == "lod_x_only" else np.maximum(rho[0], rho[1])
    unusable = ~np.isfinite(r) | (r == 0.0)
    lod = np.log2(np.where(unusable, 1.0, r)) + (0.5 if mutation == "lod_bias" else 0.0)
    T = np.where(unusable, 0.0, np.maximum(rel[0], rel[1]) / math.log(2.0) + 2.0 * EPS * (np.abs(lod) + 1.0))
    return u0, v0, lod, T, unusable


def _lod_snaps(lod, T, mips):
    lc = np.clip(lod, 0.0, mips - 1.0)
    t = lc * 256.0 + 0.5
    fl = np.floor(t)
    other = np.where(t - fl < 256.0 * T, fl - 1.0, np.where(fl + 1.0 - t < 256.0 * T, fl + 1.0, fl))
    return fl / 256.0, np.clip(other / 256.0, 0.0, mips - 1.0)


def _on_face(levels, size, mips, face, rays, mutation):
    u0, v0, lod, T, unusable = _footprint(size, face, rays, mutation)
    main, other = _lod_snaps(lod, T, mips)
    U, V = (u0 + 1.0) * 0.5, (v0 + 1.0) * 0.5
    lo, hi, mag, bad, wide, edge, corner = _trilinear(levels, size, mips, face, U, V, main, mutation)
    k = np.flatnonzero(other != main)
    if len(k):
        lo2, hi2, m2, b2, _, _, _ = _trilinear(levels, size, mips, face[k], U[k], V[k], other[k], mutation)
        lo[k], hi[k], mag[k], bad[k], wide[k] = np.fmin(lo[k], lo2), np.fmax(hi[k], hi2), np.maximum(mag[k], m2), bad[k] | b2, True
    return dict(lo=lo, hi=hi, mag=mag, bad=bad, wide=wide, edge=edge, corner=corner, lod=lod, T=T, unusable=unusable, lod_s=main,
                lod_alt=other)


# ---- the pass --------------------------------------------------------------------------------------------------------------------
def truth(g, tile, stencil, cube, size, mips, mutation=None):
    """the sky pixels (stencil == 0, row-major) of the tile: dict of
      iy, ix       their tile coordinates;  sky [h, w] the mask
      lo, hi       [n, 3] the interval;  flag [n] (FLAG_*);  wide [n] an x.8 or LOD snap alternative entered the interval;  mag [n] M
      face, lod, T, lod_s, lod_alt, edge, corner, tie    the centre face, its raw float64 LOD and tolerance, the snapped LOD and its
                   alternative, footprint leaves the face / in both axes (either level), a second face is within rounding
    stencil: [>= h, >= w] (a pitch larger than w is fine)"""
    assert mutation is None or mutation in MUTATIONS
    cam, levels = camera_of(g), levels_of(cube, size, mips)
    sky = np.asarray(stencil)[:tile.h, :tile.w] == 0
    iy, ix = np.nonzero(sky)
    n = len(iy)
    gx, gy = (tile.x0 + ix).astype(f64), (tile.y0 + iy).astype(f64)
    rays = (_rays(cam, tile, gx, gy), _rays(cam, tile, gx + 1.0, gy), _rays(cam, tile, gx, gy + 1.0))
    a = np.abs(rays[0][0])
    major, amax = _major(a), a.max(axis=1)
    out = dict(iy=iy, ix=ix, sky=sky, lo=np.full((n, 3), np.inf), hi=np.full((n, 3), -np.inf), flag=np.zeros(n, np.uint8), wide=np.zeros(n, bool),
               mag=np.zeros(n), tie=np.zeros(n, bool))
    own = np.zeros((n, 3))
    for ax in range(3):
        is_main = major == ax
        k = np.flatnonzero(is_main | (a[:, ax] >= amax * (1.0 - FACE_TIE_REL)))
        if not len(k):
            continue
        face = 2 * ax + (rays[0][0][k, ax] < 0)
        r = _on_face(levels, size, mips, face, tuple((d[k], e[k]) for d, e in rays), mutation)
        out["lo"][k], out["hi"][k] = np.fmin(out["lo"][k], r["lo"]), np.fmax(out["hi"][k], r["hi"])
        with np.errstate(invalid="ignore"):
            own[k] = np.fmax(own[k], r["hi"] - r["lo"])
        out["mag"][k] = np.maximum(out["mag"][k], r["mag"])
        out["flag"][k] |= (r["bad"] * FLAG_TAP + r["unusable"] * FLAG_RHO).astype(np.uint8)
        out["wide"][k] |= r["wide"]
        out["tie"][k] |= ~is_main[k]
        m = is_main[k]
        for name in ("lod", "T", "lod_s", "lod_alt", "edge", "corner"):
            out.setdefault(name, np.zeros(n, r[name].dtype))[k[m]] = r[name][m]
        out.setdefault("face", np.zeros(n, np.int64))[k[m]] = face[m]
    with np.errstate(invalid="ignore"):
        apart = ((out["hi"] - out["lo"]) - own).max(axis=1) > E_ROUNDINGS * EPS * out["mag"]
    out["flag"] |= ((out["tie"] & apart) * FLAG_TIE).astype(np.uint8)
    out["size"], out["mips"] = size, mips
    return out


def image_of(t, h, w, fill=0.0):
    """a half image [h, w, 4] holding the middle of every sky pixel's interval, alpha 1, `fill` elsewhere: what a correct (or, for a
    truth made with a mutation, a mistaken) resolve would store"""
    img = np.full((h, w, 4), fill, np.float16)
    with np.errstate(over="ignore", invalid="ignore"):
        img[t["iy"], t["ix"], :3] = (0.5 * (t["lo"] + t["hi"])).astype(np.float16)
    img[t["iy"], t["ix"], 3] = 1.0
    return img


def check(got, t):
    """got: half [h, >= w, 4].  -> (ratio [n]: per sky pixel the largest dist(got, [lo, hi]) / (E + S) over the channels, inf for a
    non-finite value where the truth is finite; comparable [n]: flag == 0).  The image passes when ratio[comparable] <= 1."""
    g = np.asarray(got)[t["iy"], t["ix"], :3].astype(f64)
    with np.errstate(invalid="ignore"):
        dist = np.maximum(np.maximum(t["lo"] - g, g - t["hi"]), 0.0)
        allow = (E_ROUNDINGS * EPS * t["mag"])[:, None] + 2.0 ** -11 * np.abs(g) + 2.0 ** -25
        ratio = dist / allow
    ratio = np.where(np.isfinite(g), ratio, np.where(np.isfinite(t["hi"]) & np.isfinite(t["lo"]), np.inf, 0.0))
    return np.nan_to_num(ratio, nan=np.inf).max(axis=1), t["flag"] == 0


def assert_image(got, t, what):
    """the check as an assertion; returns the worst comparable pixel as a fraction of its bound"""
    ratio, ok = check(got, t)
    worst = float(ratio[ok].max()) if ok.any() else 0.0
    k = int(np.argmax(np.where(ok, ratio, -1.0))) if ok.any() else 0
    assert worst <= 1.0, (f"{what}: {int((ratio[ok] > 1.0).sum())} of {int(ok.sum())} sky pixels outside the bound, worst {worst:.3g} x at (y, x) = "
                          f"({t['iy'][k]}, {t['ix'][k]}): got {np.asarray(got)[t['iy'][k], t['ix'][k], :3]}, lo {t['lo'][k]}, hi {t['hi'][k]}, "
                          f"face {t['face'][k]}, lod {t['lod'][k]:.6f}")
    return worst


# ---- the fp32 LOD, for measuring its distance to the float64 one ------------------------------------------------------------------
def lod_f32(g, tile, t):
    """the LOD formula in float32, one correctly rounded operation per step in the order include/pbr_hip.h writes them, on the sky pixels
    and centre faces of truth `t`: [n] float32.  near_height goes through a float64 tan rounded once (the C library's tanf may differ
    in the last place)."""
    f32 = np.float32
    M = np.array(g.InvView[:], dtype=f32).reshape(4, 4)[:3, :3]
    near = f32(g.Near)
    nh = f32(2.0) * near * f32(math.tan(float(f32(g.Fov) / f32(2.0))))
    nw = nh * f32(g.Ratio)
    W, H = f32(tile.full_w), f32(tile.full_h)

    def ray(gx, gy):
        u, v = (gx + f32(0.5)) / W, (gy + f32(0.5)) / H
        cx, cy = (f32(2.0) * u - f32(1.0)) * f32(0.5) * nw, (f32(1.0) - f32(2.0) * v) * f32(0.5) * nh
        return np.stack([(M[i, 0] * cx + M[i, 1] * cy) + M[i, 2] * near for i in range(3)], axis=-1)

    gx, gy = (tile.x0 + t["ix"]).astype(f32), (tile.y0 + t["iy"]).astype(f32)
    face = t["face"]
    with np.errstate(divide="ignore", invalid="ignore"):
        u0, v0, _ = _project(ray(gx, gy), face)
        ux, vx, _ = _project(ray(gx + f32(1.0), gy), face)
        uy, vy, _ = _project(ray(gx, gy + f32(1.0)), face)
        hs = f32(0.5) * f32(t["size"])
        rx = hs * np.sqrt((ux - u0) * (ux - u0) + (vx - v0) * (vx - v0))
        ry = hs * np.sqrt((uy - u0) * (uy - u0) + (vy - v0) * (vy - v0))
        out = np.log2(np.maximum(rx, ry))
    assert out.dtype == f32
    return out
