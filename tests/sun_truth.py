"""pbr_sun_light (include/pbr_hip.h, "Sun light with a shadow map") twice in numpy, and the band that says which pixels a test may hold
to the first of them.  This file imports no project code.

truth(...)        the rule in float64, written from the header's formulas and from brdf.hlsli:47-67 (pow(p, 5) as a power, normalize
                  as a division by the norm): the value every implementation approximates.
restate(...)      the rule in float32 in the KERNEL'S operation order: every +, -, *, /, sqrt, max and floor is one correctly rounded
                  float32 operation, in the order the header writes them.  The kernel is built without contraction and uses IEEE
                  divides and square roots only, so it equals this function bit for bit.  restate(..., defect=NAME) makes one
                  deliberate mistake (DEFECTS): the CPU tests show that each trips a named assertion.

THE BAND.  A shadow tap compares zr with a stored depth; NdotL is compared with 0.  Both are decided by rounding when the two sides
are closer than the float32 error of either, and then truth and kernel may differ by the whole contribution: such pixels have no
single truth and are SET ASIDE (`undecided`); tests cap their share.  eps = 2^-24, the unit roundoff.
  zr = q.z - bias, q.z = M2 . P + M23.  Its error has two parts.  (a) The arithmetic of the dot product, the bias and the products
  with P's own last-place error: each of the <= 8 roundings is relative to a partial sum bounded by S = |M20 P.x| + |M21 P.y| +
  |M22 P.z| + |M23| + |bias| (values <= a few units: q.z itself lies in [0, 1]), and P's components carry 3 roundings of the final
  cam + cv * zs: together <= 12 eps S.  (b) The view-space depth z_vs = Near Far / (Far - d (Far - Near)) is ill-conditioned: the
  product d (Far - Near) is rounded at magnitude ~Far and the difference that follows is Near Far / z_vs, so z_vs — and with it the
  distance |P - cam| — carries a RELATIVE error of up to 3 eps (1 + z_vs / Near) (two roundings at magnitude Far, one of the
  division), and cv a further 4 eps; moved along the view ray by that, q.z moves by |M2 . (P - cam)| times it.
  band_z = eps * (12 S + (4 + 3 (1 + z_vs / Near)) |M2 . (P - cam)|) + 12 eps S_map, the last term for the STORED depth: the raster's
  vertex stage forms the same affine map in float32 in three matrix products (<= 12 roundings of partial sums bounded as S is;
  its z / w interpolation is float64 rounded once, tests/raster_ref.py), taken as S_map = S of the receiver: the compared values
  are equal to within the band exactly when it matters.
  su, sv: (q.x + 1) * 0.5 * map_w - 0.5 has the error of q.x, <= 12 eps Sx + the ray term, times map_w / 2, plus 2 roundings of
  values <= map_w + 2: band_uv = (map / 2) (12 eps Sx + ray term of row 0 / 1) + 2 eps (map + 2).  The visibility is CONTINUOUS in su
  and sv (a footprint that moves across a texel boundary trades a tap of weight 0 for one of weight 0), with slope <= 1 per texel in
  each: an error of band_uv moves vis by at most 2 band_uv (pcf 1; pcf 3, an average, no more).  This is an error bound, not a
  set-aside rule: it is far below the 1e-4 of scale that the probe's bound allows (map <= 96: ~1e-5), and `truth` returns it.
  NdotL: N is a normalised vector of at most 4 roundings per component and the dot product 3 more, L is unit: band_n = 16 eps.
  A receiver within band_z of the depth range's ends q.z = 0 / 1 is set aside as well (pbr_sun_fit's 1 % margin keeps every receiver
  of a fitted scene away from them)."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
EPS = 2.0 ** -24
PI32, INV_PI32, EPSILON32 = f32(3.14159265359), f32(0.31830988618), f32(1e-6)
PI64, INV_PI64 = 3.14159265359, 0.31830988618      # the shader's literals (global.hlsli:4-7), not math.pi
BAND_N = 16.0 * EPS
DEFECTS = ("y_not_flipped", "half_dropped", "strict_less", "bias_added", "fresnel_ndotv", "k_ibl", "lum_permuted", "ninth_sixteenth",
           "outside_dark")


def camera_of(g):
    """the fields of a pbr_global the pass reads, from any object that has them"""
    return {"InvView": np.array(g.InvView[:], dtype=f32).reshape(4, 4), "CameraPos": np.array(g.CameraPos[:], dtype=f32),
            "Near": f32(g.Near), "Far": f32(g.Far), "Fov": f32(g.Fov), "Ratio": f32(g.Ratio)}


def make_sun(direction, luminance, M=None, bias=(0.0, 0.0), pcf=3):
    d = np.asarray(direction, dtype=f64)
    d = (d / math.sqrt(float((d * d).sum()))).astype(f32)
    return {"Direction": d, "Luminance": np.broadcast_to(np.asarray(luminance, dtype=f32), (3,)).copy(),
            "M": (np.eye(4, dtype=f32) if M is None else np.asarray(M, dtype=f32).reshape(4, 4)),
            "bias_const": f32(bias[0]), "bias_slope": f32(bias[1]), "pcf": int(pcf)}


def _bytes(plane, k):
    return ((np.asarray(plane).astype(np.uint32) >> np.uint32(8 * k)) & np.uint32(255))


def _pixel_grid(tile):
    gx = (tile.x0 + np.arange(tile.w))[None, :] + np.zeros((tile.h, 1), dtype=np.int64)
    gy = (tile.y0 + np.arange(tile.h))[:, None] + np.zeros((1, tile.w), dtype=np.int64)
    return gx, gy


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _tap_planes(depth_map, ix, iy, offsets):
    """stored depth and inside-the-map mask of the taps (ix + i, iy + j) for (i, j) in offsets: dict (i, j) -> (stored, inside)"""
    mh, mw = depth_map.shape
    out = {}
    for (i, j) in offsets:
        tx, ty = ix + i, iy + j
        inside = (tx >= 0) & (tx < mw) & (ty >= 0) & (ty < mh)
        out[(i, j)] = (depth_map[np.clip(ty, 0, mh - 1), np.clip(tx, 0, mw - 1)], inside)
    return out


def _offsets(pcf):
    return [(i, j) for j in ((0, 1) if pcf == 1 else (-1, 0, 1, 2)) for i in ((0, 1) if pcf == 1 else (-1, 0, 1, 2))]


def _filter(t, wx, wy, pcf, one, ninth):
    """the visibility of the lit / dark taps t[(i, j)] (arrays of 0 / 1 in the caller's precision)"""
    lerp = lambda a, b, w: a + (b - a) * w
    if pcf == 1:
        return lerp(lerp(t[(0, 0)], t[(1, 0)], wx), lerp(t[(0, 1)], t[(1, 1)], wx), wy)
    hrow = {j: [lerp(t[(i, j)], t[(i + 1, j)], wx) for i in (-1, 0, 1)] for j in (-1, 0, 1, 2)}
    s = one * 0
    for j in (-1, 0, 1):
        for i in range(3):
            s = s + lerp(hrow[j][i], hrow[j + 1][i], wy)
    return s * ninth


def restate(cam, tile, gb, sun, depth_map=None, defect=None, details=None):
    """float32 [h, w, 4]: what pbr_sun_light stores in contrib_f32, operation for operation.  details: a dict that receives vis, NdotL,
    lit (stencil > 0 and NdotL > 0) and zr."""
    assert defect is None or defect in DEFECTS
    with np.errstate(all="ignore"):
        one = f32(1.0)
        inv255 = one / f32(255.0)
        IV, C = cam["InvView"], cam["CameraPos"]
        near, far = cam["Near"], cam["Far"]
        near_height = f32(2.0 * float(near) * math.tan(float(cam["Fov"]) / 2.0))
        near_width = near_height * cam["Ratio"]
        A, B, Cc = gb["A"], gb["B"], gb["C"]
        depth = np.asarray(gb["depth"], dtype=f32)
        on = np.asarray(gb["stencil"]) > 0
        ex, ey = _bytes(B, 0).astype(f32) * inv255, _bytes(B, 1).astype(f32) * inv255
        dx, dy = ex * f32(2.0) - one, ey * f32(2.0) - one
        dz = one - np.abs(dx) - np.abs(dy)
        sgn = lambda v: np.where(v < 0, f32(-1.0), one)
        fold = dz < 0
        nx, ny = sgn(dx) * (one - np.abs(dy)), sgn(dy) * (one - np.abs(dx))
        dx, dy = np.where(fold, nx, dx), np.where(fold, ny, dy)
        ln = np.sqrt(_dot((dx, dy, dz), (dx, dy, dz)))
        N = (dx / ln, dy / ln, dz / ln)
        L = tuple(f32(v) for v in sun["Direction"])
        NdotL = _dot(N, L)
        lit = on & (NdotL > 0)
        gx, gy = _pixel_grid(tile)
        u = (gx.astype(f32) + f32(0.5)) / f32(tile.full_w)
        v = (gy.astype(f32) + f32(0.5)) / f32(tile.full_h)
        cvx = (f32(2.0) * u - one) * f32(0.5) * near_width
        cvy = (one - f32(2.0) * v) * f32(0.5) * near_height
        cv = [(IV[i, 0] * cvx + IV[i, 1] * cvy) + IV[i, 2] * near for i in range(3)]
        z_vs = (near * far) / (far - depth * (far - near))
        zs = z_vs / near
        P = [C[i] + cv[i] * zs for i in range(3)]
        w = [C[i] - P[i] for i in range(3)]
        lw = np.sqrt(_dot(w, w))
        V = [w[i] / lw for i in range(3)]
        rough, metal = _bytes(Cc, 0).astype(f32) * inv255, _bytes(Cc, 1).astype(f32) * inv255
        alb = [_bytes(A, k).astype(f32) * inv255 for k in range(3)]
        h = [L[i] + V[i] for i in range(3)]
        lh = np.sqrt(_dot(h, h))
        H = [h[i] / lh for i in range(3)]
        NdotV, NdotH = np.maximum(_dot(N, V), f32(0.0)), np.maximum(_dot(N, H), f32(0.0))
        pw = np.maximum(one - (NdotV if defect == "fresnel_ndotv" else NdotL), EPSILON32)
        p5 = ((pw * pw) * (pw * pw)) * pw
        ra = rough * rough
        t = (NdotH * NdotH) * (ra * ra - one) + one
        D = (ra * ra) / np.maximum((PI32 * t) * t, EPSILON32)
        k = (rough * rough) * f32(0.5) if defect == "k_ibl" else ((rough + one) * (rough + one)) * f32(0.125)
        G = (NdotV / np.maximum(NdotV * (one - k) + k, EPSILON32)) * (NdotL / np.maximum(NdotL * (one - k) + k, EPSILON32))
        den = np.maximum((f32(4.0) * NdotL) * NdotV, f32(0.0001))
        lum = sun["Luminance"][[1, 2, 0]] if defect == "lum_permuted" else sun["Luminance"]
        c = []
        for ch in range(3):
            F0 = f32(0.04) + (alb[ch] - f32(0.04)) * metal
            F = F0 + (one - F0) * p5
            Kd = (one - F) * (one - metal)
            brdf = (Kd * alb[ch]) * INV_PI32 + ((F * D) * G) / den
            c.append((brdf * f32(lum[ch])) * NdotL)
        vis = np.ones(depth.shape, f32)
        zr = np.zeros(depth.shape, f32)
        if depth_map is not None:
            M = sun["M"]
            q = [((M[i, 0] * P[0] + M[i, 1] * P[1]) + M[i, 2] * P[2]) + M[i, 3] for i in range(3)]
            bias = sun["bias_const"] + sun["bias_slope"] * (one - NdotL)
            zr = (q[2] + bias) if defect == "bias_added" else (q[2] - bias)
            mh, mw = depth_map.shape
            half = f32(0.0) if defect == "half_dropped" else f32(0.5)
            su = ((q[0] + one) * f32(0.5)) * f32(mw) - half
            sv = (((one + q[1]) if defect == "y_not_flipped" else (one - q[1])) * f32(0.5)) * f32(mh) - half
            ranged = (q[2] >= 0) & (q[2] <= 1) & (su >= -2) & (su < f32(mw) + one) & (sv >= -2) & (sv < f32(mh) + one)
            fu, fv = np.floor(su), np.floor(sv)
            wx, wy = su - fu, sv - fv
            ix = np.where(ranged, fu, 0).astype(np.int64)
            iy = np.where(ranged, fv, 0).astype(np.int64)
            taps = {}
            for key, (stored, inside) in _tap_planes(np.asarray(depth_map, dtype=f32), ix, iy, _offsets(sun["pcf"])).items():
                passed = (zr < stored) if defect == "strict_less" else (zr <= stored)
                taps[key] = np.where(inside, passed, defect != "outside_dark").astype(f32)
            ninth = one / f32(16.0) if defect == "ninth_sixteenth" else one / f32(9.0)
            vis = np.where(ranged, _filter(taps, wx, wy, sun["pcf"], one, ninth), one).astype(f32)
        out = np.zeros(depth.shape + (4,), f32)
        for ch in range(3):
            out[..., ch] = np.where(lit, c[ch] * vis, f32(0.0))
        out[..., 3] = np.where(lit, one, f32(0.0))
        if details is not None:
            details.update(vis=np.where(lit, vis, f32(0.0)), NdotL=NdotL, lit=lit, zr=zr)
        return out


def truth(cam, tile, gb, sun, depth_map=None):
    """The rule in float64.  Returns a dict: contrib [h, w, 3], unshadowed [h, w, 3] (c, the contribution at vis = 1), vis, NdotL, lit
    (stencil > 0 and NdotL > 0), undecided (a tap or NdotL inside its band), band_z, band_vis (the bound on vis's own error from su /
    sv), position [h, w, 3] and q [h, w, 3]."""
    with np.errstate(all="ignore"):
        IV, C = cam["InvView"].astype(f64), cam["CameraPos"].astype(f64)
        near, far = float(cam["Near"]), float(cam["Far"])
        near_height = 2.0 * near * math.tan(float(cam["Fov"]) / 2.0)
        near_width = near_height * float(cam["Ratio"])
        depth = np.asarray(gb["depth"]).astype(f64)
        on = np.asarray(gb["stencil"]) > 0
        e = np.stack([_bytes(gb["B"], 0), _bytes(gb["B"], 1)], axis=-1).astype(f64) / 255.0
        d = np.concatenate([e * 2.0 - 1.0, np.zeros(depth.shape + (1,))], axis=-1)
        d[..., 2] = 1.0 - np.abs(d[..., 0]) - np.abs(d[..., 1])
        fold = d[..., 2] < 0
        sgn = lambda v: np.where(v < 0, -1.0, 1.0)
        nx, ny = sgn(d[..., 0]) * (1.0 - np.abs(d[..., 1])), sgn(d[..., 1]) * (1.0 - np.abs(d[..., 0]))
        d[..., 0], d[..., 1] = np.where(fold, nx, d[..., 0]), np.where(fold, ny, d[..., 1])
        N = d / np.linalg.norm(d, axis=-1, keepdims=True)
        L = sun["Direction"].astype(f64)
        NdotL = N @ L
        lit = on & (NdotL > 0)
        gx, gy = _pixel_grid(tile)
        u, v = (gx + 0.5) / tile.full_w, (gy + 0.5) / tile.full_h
        cvv = np.stack([(2.0 * u - 1.0) * 0.5 * near_width, (1.0 - 2.0 * v) * 0.5 * near_height, np.full(u.shape, near)], axis=-1)
        cv = cvv @ IV[:3, :3].T
        z_vs = near * far / (far - depth * (far - near))
        P = C + cv * (z_vs / near)[..., None]
        V = C - P
        V = V / np.linalg.norm(V, axis=-1, keepdims=True)
        rough, metal = _bytes(gb["C"], 0).astype(f64) / 255.0, _bytes(gb["C"], 1).astype(f64) / 255.0
        alb = np.stack([_bytes(gb["A"], k) for k in range(3)], axis=-1).astype(f64) / 255.0
        H = L + V
        H = H / np.linalg.norm(H, axis=-1, keepdims=True)
        NdotV = np.maximum((N * V).sum(-1), 0.0)
        NdotH = np.maximum((N * H).sum(-1), 0.0)
        F0 = 0.04 + (alb - 0.04) * metal[..., None]
        F = F0 + (1.0 - F0) * (np.maximum(1.0 - NdotL, 1e-6) ** 5)[..., None]
        a = rough * rough
        t = NdotH * NdotH * (a * a - 1.0) + 1.0
        D = a * a / np.maximum(PI64 * t * t, 1e-6)
        k = (rough + 1.0) * (rough + 1.0) / 8.0
        G = (NdotV / np.maximum(NdotV * (1.0 - k) + k, 1e-6)) * (NdotL / np.maximum(NdotL * (1.0 - k) + k, 1e-6))
        Kd = (1.0 - F) * (1.0 - metal)[..., None]
        brdf = Kd * alb * INV_PI64 + F * (D * G / np.maximum(4.0 * NdotL * NdotV, 0.0001))[..., None]
        c = brdf * sun["Luminance"].astype(f64) * NdotL[..., None]
        vis = np.ones(depth.shape)
        undecided = on & (np.abs(NdotL) <= BAND_N)
        band_z = np.zeros(depth.shape)
        band_vis = np.zeros(depth.shape)
        q = np.zeros(depth.shape + (3,))
        if depth_map is not None:
            M = sun["M"].astype(f64)
            q = P @ M[:3, :3].T + M[:3, 3]
            bias = float(sun["bias_const"]) + float(sun["bias_slope"]) * (1.0 - NdotL)
            zr = q[..., 2] - bias
            mh, mw = depth_map.shape
            su = (q[..., 0] + 1.0) * 0.5 * mw - 0.5
            sv = (1.0 - q[..., 1]) * 0.5 * mh - 0.5
            ranged = (q[..., 2] >= 0) & (q[..., 2] <= 1) & (su >= -2) & (su < mw + 1) & (sv >= -2) & (sv < mh + 1)
            ray = P - C
            cond = 4.0 + 3.0 * (1.0 + z_vs / near)
            S = [np.abs(M[i, :3] * P).sum(-1) + abs(M[i, 3]) for i in range(3)]
            ray_i = [np.abs(ray @ M[i, :3]) for i in range(3)]
            band_z = EPS * (12.0 * (S[2] + np.abs(bias)) + cond * ray_i[2]) + 12.0 * EPS * S[2]
            band_uv = [0.5 * m * EPS * (12.0 * S[i] + cond * ray_i[i]) + 2.0 * EPS * (m + 2) for i, m in ((0, mw), (1, mh))]
            band_vis = 2.0 * (band_uv[0] + band_uv[1])
            fu, fv = np.floor(su), np.floor(sv)
            wx, wy = su - fu, sv - fv
            ix = np.where(ranged, fu, 0).astype(np.int64)
            iy = np.where(ranged, fv, 0).astype(np.int64)
            taps = {}
            close = np.zeros(depth.shape, bool)
            for key, (stored, inside) in _tap_planes(np.asarray(depth_map).astype(f64), ix, iy, _offsets(sun["pcf"])).items():
                taps[key] = np.where(inside, zr <= stored, True).astype(f64)
                close |= inside & (np.abs(zr - stored) <= band_z)
            vis = np.where(ranged, _filter(taps, wx, wy, sun["pcf"], 1.0, 1.0 / 9.0), 1.0)
            edge = (np.abs(q[..., 2]) <= band_z) | (np.abs(q[..., 2] - 1.0) <= band_z)
            undecided |= lit & ((ranged & close) | edge)
        contrib = np.where(lit[..., None], c * vis[..., None], 0.0)
        return {"contrib": contrib, "unshadowed": np.where(lit[..., None], c, 0.0), "vis": np.where(lit, vis, 0.0), "NdotL": NdotL,
                "lit": lit, "undecided": undecided, "band_z": band_z, "band_vis": band_vis, "position": P, "q": q, "on": on}


# the probe's bound, the shade's own form (tests/shade_checks.py): per decided pixel and channel
#   |got - f64| <= 1e-4 * scale + 4 * |float32 restatement - f64|,   scale = the largest channel of the pixel's UNSHADOWED contribution
F32_REL, RESTATEMENT_FACTOR = 1e-4, 4.0


def probe_worst(got, tr, restated):
    """(worst ratio of |got - truth| to its bound over the decided geometry pixels, the number of such pixels); got and restated are
    float32 [h, w, 4] probe images, tr = truth(...).  Pixels the rule leaves untouched (stencil 0, NdotL <= 0) must be exactly 0 with
    alpha 0, lit ones carry alpha 1: that part is asserted here."""
    got = np.asarray(got)
    assert got.shape == restated.shape and np.isfinite(got).all()
    decided = ~tr["undecided"]
    dark = decided & ~tr["lit"]
    assert not got[dark].any(), "a pixel without geometry or with NdotL <= 0 carries a contribution"
    use = decided & tr["lit"]
    assert (got[use][:, 3] == 1.0).all(), "a lit pixel's probe alpha is not 1"
    scale = tr["unshadowed"][use].max(axis=-1, keepdims=True)
    err = np.abs(got[use][:, :3].astype(f64) - tr["contrib"][use])
    bound = F32_REL * scale + RESTATEMENT_FACTOR * np.abs(restated[use][:, :3].astype(f64) - tr["contrib"][use])
    ratio = err / np.maximum(bound, 1e-300)
    return (float(ratio.max()) if ratio.size else 0.0), int(use.sum())


def classes(tr):
    """shares, among the geometry pixels, of the undecided pixels and of the decided lit (vis == 1), fully shadowed (vis == 0) and
    penumbra (in between) pixels with NdotL > 0"""
    n = max(int(tr["on"].sum()), 1)
    use = tr["lit"] & ~tr["undecided"]
    v = tr["vis"][use]
    return {"undecided": float(tr["undecided"].sum()) / n, "lit": float((v == 1.0).sum()) / n, "shadowed": float((v == 0.0).sum()) / n,
            "penumbra": float(((v > 0.0) & (v < 1.0)).sum()) / n}


def sun_fit(direction, box_min, box_max, map_w, map_h):
    """pbr_sun_fit in float64, every matrix entry rounded once to float32: (View, Projection, InvProjection, LightViewProj) as 4 x 4
    float32 arrays and the light-space extents (l, r, b, t, n, f) after widening"""
    d = np.asarray(direction, dtype=f32).astype(f64)
    d = d / math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    z = -d
    up = np.array([1.0, 0.0, 0.0]) if abs(d[1]) > 0.999 else np.array([0.0, 1.0, 0.0])
    x = np.array([up[1] * z[2] - up[2] * z[1], up[2] * z[0] - up[0] * z[2], up[0] * z[1] - up[1] * z[0]])
    x = x / math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
    y = np.array([z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]])
    axes = [x, y, z]
    mn, mx = np.asarray(box_min, dtype=f32).astype(f64), np.asarray(box_max, dtype=f32).astype(f64)
    lo, hi = [], []
    for a in axes:
        vals = [(a[0] * (mx[0] if c & 1 else mn[0]) + a[1] * (mx[1] if c & 2 else mn[1])) + a[2] * (mx[2] if c & 4 else mn[2]) for c in range(8)]
        l_, h_ = min(vals), max(vals)
        if h_ - l_ < 1e-6:
            mid = (l_ + h_) * 0.5
            l_, h_ = mid - 0.5e-6, mid + 0.5e-6
        lo.append(l_)
        hi.append(h_)
    ex, ey, ez = (hi[0] - lo[0]) / (map_w - 2), (hi[1] - lo[1]) / (map_h - 2), 0.01 * (hi[2] - lo[2])
    l, r, b, t, n, f = lo[0] - ex, hi[0] + ex, lo[1] - ey, hi[1] + ey, lo[2] - ez, hi[2] + ez
    V = np.eye(4, dtype=f32)
    V[:3, :3] = np.array(axes).astype(f32)
    Pm = np.eye(4, dtype=f32)
    Pm[0, 0], Pm[0, 3] = f32(2.0 / (r - l)), f32(-(r + l) / (r - l))
    Pm[1, 1], Pm[1, 3] = f32(2.0 / (t - b)), f32(-(t + b) / (t - b))
    Pm[2, 2], Pm[2, 3] = f32(1.0 / (f - n)), f32(-n / (f - n))
    IP = np.eye(4, dtype=f32)
    IP[0, 0], IP[0, 3] = f32((r - l) / 2.0), f32((r + l) / 2.0)
    IP[1, 1], IP[1, 3] = f32((t - b) / 2.0), f32((t + b) / 2.0)
    IP[2, 2], IP[2, 3] = f32(f - n), f32(n)
    lvp = np.zeros((4, 4), f32)
    for i in range(4):
        for j in range(4):
            acc = 0.0
            for k in range(4):
                acc = acc + float(Pm[i, k]) * float(V[k, j])
            lvp[i, j] = f32(acc)
    return V, Pm, IP, lvp, (l, r, b, t, n, f)


def assert_probe(got, tr, restated, what):
    """the probe's bound as an assertion ("probe bound" in its message); returns the worst ratio"""
    worst, n = probe_worst(got, tr, restated)
    assert n > 0, f"{what}: no decided lit pixel"
    assert worst <= 1.0, f"{what}: probe bound missed, a pixel is {worst:.3g} x its bound from the float64 truth ({n} pixels)"
    return worst
