"""The inputs on which the sky resolve is held to tests/sky_truth.py — the smallest at which each piece of the pass can go wrong — and
the conditions they have to meet, asserted on what actually runs (assert_coverage, from the truth's own per-pixel analysis).

Cameras: the four of camera_cases and the ten of sky_bc6h_cases (pitch, roll, straight up and down, wide), under their names.  ONE
camera is added, `diagonal`: none of those can put a ray on a face diagonal — the only axis-aligned ones are `default`, whose
tan(Fov / 2) Ratio ndc_x never reaches 1 at a pixel centre of the frames below, and the narrow `corner` —, so the tie case uses an
unrotated camera of Fov pi / 2 on an 8 x 6 tile of a 97 x 64 frame, where the pixel centres of column 80 have ndc_x = 64 / 97 =
1 / Ratio and |d.x| = |d.z| in exact arithmetic.

Cubes: fp32 RGBA, values in [0, 1000].  `smooth` is a smooth function of the direction with a chain from the oracle's cube_gen_mips;
`checker` is a per-texel checker of contrast 50 : 1, every face a hue of its own, and — stated here because a box filter would flatten
it — every LEVEL of its chain is such a checker too, dimmer by a tenth per level, so that one wrong tap, face or level shows at once;
`const` holds (0.7, 11.0, 65503.9) on every level; `levels` holds an unrelated constant per level (the level weight is read off the
output); level_coded() holds the level's number (the output IS the snapped LOD, exact in half below 8)."""
import numpy as np

import camera_cases
import sky_bc6h_cases
from direct12pbrrenderer_amd import scene
from direct12pbrrenderer_amd.structs import Tile

CHAINS = ((1, 1), (2, 2), (4, 3), (20, 3), (64, 7))      # 20^2 x 3: not a power of two, and the chain ends at 5^2
CONST = (0.7, 11.0, 65503.9)
LEVEL_VALUES = ((3.0, 640.0, 17.0), (911.0, 2.0, 260.0), (55.0, 130.0, 999.0))
HUES = ((1.0, 0.1, 0.1), (0.1, 1.0, 0.1), (0.1, 0.1, 1.0), (1.0, 1.0, 0.1), (1.0, 0.1, 1.0), (0.1, 1.0, 1.0))
A, B, TINY, SMALL, WIDE = (96, 64, None, 0, 0), (48, 32, None, 0, 0), (2, 2, None, 0, 0), (8, 6, None, 0, 0), (160, 90, None, 0, 0)
RAGGED = camera_cases.SHADE_SHAPES[1]                    # 200 x 37 at (328, 91) of 640 x 360
DIAGONAL = (8, 6, (97, 64), 76, 29)
assert RAGGED == (200, 37, (640, 360), 328, 91)

# (cube kind, (size, mips), camera, (w, h, full, x0, y0))
#
# The x.8 snap rule sets aside a share of the pixels that grows with the level's edge (16 ulps of c . 256 on either side of a step:
# about 3 % of the pixels of a 64^2 level, 1.5 % of a 32^2 one) and the LOD rule about 2 % of the pixels between two levels at these
# frame sizes, so a case whose pixels mostly blend levels 0 and 1 of the 64^2 chain cannot stay under the 5 % cap of
# test_sky_truth_cpu.py.  The 64^2 chain therefore meets its level pairs in cases chosen for it: magnified 96 x 64 frames whose
# corners reach into (0, 1) and (1, 2), `default` at 48 x 32 (LOD 0.21 on every pixel, no snap alternative) and the small wide frames
# for the pairs above; the smaller chains take the full list.
CASES = []
_SMALL_CHAIN_FRAMES = (("pitch_roll", A), ("default", B), ("up", B), ("down", B), ("roll_only", B), ("pitch_only", B), ("plus_x", B),
                       ("minus_x", B), ("wide_a", TINY), ("wide_d", SMALL), ("wide_b", SMALL), ("wide_c", TINY), ("wide_e", SMALL), ("wide_a", B))
_FULL_CHAIN_FRAMES = (("pitch_roll", A), ("default", B), ("up", A), ("wide_e", A), ("wide_d", A), ("minus_x", A), ("wide_a", TINY),
                      ("wide_d", SMALL), ("wide_b", SMALL), ("wide_c", TINY), ("wide_e", SMALL), ("wide_a", SMALL), ("pitch_only", SMALL),
                      ("pitch_only", TINY))
for _chain in CHAINS:
    for _k, (_name, _frame) in enumerate(_FULL_CHAIN_FRAMES if _chain == (64, 7) else _SMALL_CHAIN_FRAMES):
        CASES.append((("checker", "smooth")[_k % 2], _chain, _name, _frame))
CASES += [("checker", (64, 7), "pitch_roll", RAGGED), ("smooth", (4, 3), "pitch_roll", RAGGED), ("checker", (20, 3), "default", WIDE),
          ("checker", (4, 3), "wide_e", B), ("checker", (20, 3), "wide_b", B),
          ("const", (4, 3), "wide_d", SMALL), ("const", (64, 7), "wide_b", SMALL), ("const", (20, 3), "up", B), ("const", (1, 1), "pitch_roll", B),
          ("levels", (4, 3), "wide_a", SMALL), ("levels", (4, 3), "wide_b", SMALL), ("levels", (4, 3), "pitch_roll", B),
          ("checker", (4, 3), "diagonal", DIAGONAL), ("smooth", (64, 7), "diagonal", DIAGONAL)]
# where each mistake of sky_truth.MUTATIONS has to show (test_sky_truth_cpu.py); no_snap on a steep checker
MUTATION_CASES = {
    "lod_bias": ("levels", (4, 3), "wide_a", SMALL),
    "lod_x_only": ("levels", (4, 3), "wide_b", SMALL),
    "clamp_to_edge": ("checker", (4, 3), "pitch_roll", A),
    "corner_x_first": ("checker", (2, 2), "up", B),
    "swap_faces_2_3": ("checker", (20, 3), "up", B),
    "no_snap": ("checker", (4, 3), "pitch_roll", A),
}
assert all(c in CASES for c in MUTATION_CASES.values())


def make_global(name, full_w, full_h):
    if name == "diagonal":
        return scene.make_global(scene.Camera(scene.f32(scene.PI) / scene.f32(2.0), full_w, full_h, 0.1, 100.0), full_w, full_h)
    return sky_bc6h_cases.make_global(name, full_w, full_h)


def _texel_dirs(s):
    """unit directions [6, s, s, 3] of a level's texel centres"""
    c = (np.arange(s) + 0.5) / s * 2.0 - 1.0
    v, u = np.meshgrid(c, c, indexing="ij")
    one = np.ones_like(u)
    d = np.stack([np.stack(t, axis=-1) for t in ((one, -v, -u), (-one, -v, u), (u, one, v), (u, -one, -v), (u, -v, one), (-u, -v, -one))])
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _level_sizes(size, mips):
    return [size >> l for l in range(mips)]


def make_cube(orc, kind, size, mips):
    """float32 [texels, 4] in the pbr_cube_f32 layout, alpha 1"""
    levels = []
    for l, s in enumerate(_level_sizes(size, mips)):
        t = np.ones((6, s, s, 4), np.float32)
        if kind == "smooth":
            x, y, z = np.moveaxis(_texel_dirs(s), -1, 0)
            t[..., 0] = 500.0 + 480.0 * np.sin(2.2 * x + 0.7) * np.cos(1.7 * y - 0.4)
            t[..., 1] = 400.0 + 390.0 * np.sin(2.9 * z - 1.1 + 0.8 * x)
            t[..., 2] = 10.0 + 9.0 * np.cos(3.1 * y + 1.3 * z)
        elif kind == "checker":
            yy, xx = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")
            amp = np.where((xx + yy + l) % 2 == 0, 1000.0, 20.0) * (1.0 - 0.1 * l)
            t[..., :3] = amp[None, :, :, None] * np.asarray(HUES)[:, None, None, :]
        elif kind == "const":
            t[..., :3] = np.float32(CONST)
        elif kind == "levels":
            t[..., :3] = np.float32(LEVEL_VALUES[l])
        else:
            raise ValueError(kind)
        levels.append(t.reshape(-1, 4))
    cube = np.ascontiguousarray(np.concatenate(levels), dtype=np.float32)
    if kind == "smooth":
        orc.cube_gen_mips(cube, size, mips)
    assert np.isfinite(cube).all() and cube[:, :3].min() >= 0.0 and (cube[:, :3].max() <= 1000.0 or kind == "const")
    return cube


def level_coded(size, mips):
    """every texel of level l holds l: the resolve's output is its snapped LOD"""
    return np.concatenate([np.full((6 * s * s, 4), float(l), np.float32) for l, s in enumerate(_level_sizes(size, mips))])


def case_inputs(case):
    """-> (kind, size, mips, Global, Tile, stencil uint8 [h, w]): a seeded tenth of the pixels is geometry; the ragged tile carries two
    solid blocks of it as well"""
    kind, (size, mips), name, (w, h, full, x0, y0) = case
    full_w, full_h = full if full else (w, h)
    rng = np.random.default_rng(size * 1000 + w * 7 + h)
    stencil = (rng.random((h, w)) < 0.1).astype(np.uint8) * rng.integers(1, 255, (h, w), dtype=np.uint8)
    if full:
        stencil[: h // 3, w // 2: w // 2 + w // 8] = 7
        stencil[h // 2:, : w // 10] = 255
    if w * h <= 64:
        stencil[:] = 0
        stencil[h - 1, w - 1] = 3 if w * h > 4 else 0
    return kind, size, mips, make_global(name, full_w, full_h), Tile(x0, y0, w, h, full_w, full_h), stencil


# ---- what the cases exercise, from the truth's own analysis of each ----------------------------------------------------------------
def coverage(truths):
    """truths: {case: sky_truth.truth(...)} of every case -> the counts assert_coverage() looks at"""
    faces, edge, corner, ties, pairs = set(), 0, 0, 0, {c: set() for c in CHAINS}
    lod0, top = 0, {c: 0 for c in CHAINS}
    for case, t in truths.items():
        chain = case[1]
        faces |= set(np.unique(t["face"]).tolist())
        edge += int(t["edge"].sum())
        corner += int(t["corner"].sum())
        sure = t["lod_alt"] == t["lod_s"]
        lod0 += int(((t["lod"] <= 0.0) & sure).sum())
        top[chain] += int(((t["lod"] >= chain[1] - 1.0) & sure).sum())
        frac = t["lod_s"] % 1.0
        part = sure & (frac >= 1.0 / 16.0) & (frac <= 15.0 / 16.0)
        pairs[chain] |= set(np.floor(t["lod_s"][part]).astype(int).tolist())
        if case[2] in ("default", "corner", "diagonal"):
            ties += int(t["tie"].sum())
    return dict(faces=faces, edge=edge, corner=corner, lod0=lod0, top=top, pairs=pairs, ties=ties)


def assert_coverage(c):
    assert c["faces"] == {0, 1, 2, 3, 4, 5}, c["faces"]                                   # all six faces are a centre face
    assert c["edge"] >= 200 and c["corner"] >= 8, (c["edge"], c["corner"])                # footprints across an edge, and off in both axes
    assert c["lod0"] >= 100, c["lod0"]                                                    # LOD clamped at 0
    assert c["top"][(64, 7)] >= 4 and c["top"][(20, 3)] >= 20 and c["top"][(4, 3)] >= 4, c["top"]   # clamped at mips - 1: full and short chain
    assert c["pairs"][(4, 3)] >= {0, 1} and c["pairs"][(64, 7)] >= {0, 1, 2, 3, 4, 5}, c["pairs"]    # fractional on every adjacent pair
    assert c["ties"] >= 4, c["ties"]                                                      # an axis-aligned camera's rays on a face diagonal
