"""CPU checks of the textured raster's pinned sampler (include/pbr_hip.h) through its restatement (tests/raster_tex_ref.py): the
decode tables against the kernel's, known answers of the filter, LOD and swizzles, the normal-map frame, and the ABI layouts."""
import ctypes as C
import os
import re

import numpy as np

import raster_tex_ref as rt
from direct12pbrrenderer_amd import scene, structs
from direct12pbrrenderer_amd.structs import (DRAW_MAPS_DTYPE, NO_MAP, TEX_B8G8R8A8_UNORM, TEX_B8G8R8A8_UNORM_SRGB, TEX_R8_UNORM,
                                             TEX_R8G8B8A8_UNORM, Texture2D)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def header_table(name):
    src = open(os.path.join(ROOT, "direct12pbrrenderer_amd", "csrc", "texel_decode.hpp")).read()
    body = re.search(r"%s\[256\] = \{(.*?)\};" % name, src, re.S).group(1)
    return np.array([float.fromhex(t.strip().rstrip("f")) for t in body.split(",") if t.strip()], dtype=f32)


def test_decode_tables_match_the_kernel():
    assert np.array_equal(header_table("kUnorm8").view(np.uint32), rt.unorm_table().view(np.uint32))
    assert np.array_equal(header_table("kSrgb8").view(np.uint32), rt.srgb_table().view(np.uint32))


def test_srgb_table_endpoints():
    s = rt.srgb_table()
    assert s[0] == 0.0 and s[255] == 1.0
    assert s[10] == f32(10 / 255 / 12.92)                        # linear segment (10 / 255 <= 0.04045)
    assert s[11] == f32(((11 / 255 + 0.055) / 1.055) ** 2.4)     # first value on the power segment
    assert (np.diff(s) > 0).all()
    u = rt.unorm_table()
    assert u[0] == 0.0 and u[255] == 1.0 and u[51] == f32(0.2)


def test_fma32_single_rounding():
    rng = np.random.default_rng(0)
    a, b, c = (rng.uniform(-2, 2, 20000).astype(f32) for _ in range(3))
    got = rt.fma32(a, b, c)
    # the exact value a b + c as a rational, rounded once: compare with float64 where float64 is exact enough to decide
    ref = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)
    assert (got == ref).mean() > 0.999
    # a case where rounding twice goes wrong: 1 + 2^-24 + 2^-60 (float64 rounds onto the float32 midpoint)
    x = rt.fma32(f32(1.0 + 2.0 ** -23), f32(1.0 + 2.0 ** -23), f32(-(2.0 ** -23)))   # 1 + 2^-23 + 2^-46
    assert x == f32(1.0 + 2.0 ** -23)
    y = rt.fma32(f32(1.0 + 2.0 ** -12), f32(1.0 + 2.0 ** -12), f32(-(2.0 ** -11)))      # 1 + 2^-24 exactly: a tie, to even
    assert y == f32(1.0)


def tex_rgba(levels, fmt=TEX_R8G8B8A8_UNORM):
    return rt.texture_dict([np.asarray(l, np.uint8) for l in levels], fmt)


def test_texel_centres_and_wrap_seams():
    lv = np.zeros((4, 4, 4), np.uint8)
    lv[..., 0] = np.arange(16).reshape(4, 4) * 16
    t = tex_rgba([lv])
    dec = rt.decode_levels(t)
    z = np.zeros(1, f32)
    for y in range(4):
        for x in range(4):
            u, v = f32((x + 0.5) / 4), f32((y + 0.5) / 4)
            s = rt.sample(t, dec, np.array([u]), np.array([v]), z, z, z, z)
            assert s[0, 0] == f32(lv[y, x, 0] / 255.0)                      # a texel centre is that texel
    # the seam: u = 0 lies half-way between texel 3 and texel 0 of the same row (wrap)
    s = rt.sample(t, dec, np.array([f32(0.0)]), np.array([f32(0.125)]), z, z, z, z)
    assert np.isclose(s[0, 0], (lv[0, 3, 0] + lv[0, 0, 0]) / 2 / 255.0, atol=1e-6)
    # whole periods: u + 7, v - 3 sample the same place, far outside [0, 1] too
    a = rt.sample(t, dec, np.array([f32(0.3)]), np.array([f32(0.6)]), z, z, z, z)
    b = rt.sample(t, dec, np.array([f32(7.3)]), np.array([f32(-2.4)]), z, z, z, z)
    assert np.allclose(a, b, atol=1e-5)


def test_lod_exact_powers_and_clamps():
    t = {"width": 256, "height": 64, "mips": 7}
    for k in range(7):
        d = np.array([f32(2.0 ** k / 256)])
        assert rt.lod(t, d, d * 0, d * 0, d * 0)[0] == k                       # |ddx| = 2^k texels
        dv = np.array([f32(2.0 ** k / 64)])
        assert rt.lod(t, dv * 0, dv * 0, dv * 0, dv)[0] == k                   # |ddy| along v, scaled by the height
    z = np.zeros(1, f32)
    assert rt.lod(t, z, z, z, z)[0] == 0                                       # rho 0
    assert rt.lod(t, np.array([f32(np.nan)]), z, z, z)[0] == 0                 # NaN
    assert rt.lod(t, np.array([f32(1e9)]), z, z, z)[0] == 6                    # clamped to mips - 1
    assert rt.lod(t, np.array([f32(0.1 / 256)]), z, z, z)[0] == 0              # magnification


def test_swizzles():
    texel = np.array([[[10, 20, 30, 40]]], np.uint8)
    rgba = rt.decode_levels(tex_rgba([texel], TEX_R8G8B8A8_UNORM))[0][0, 0]
    bgra = rt.decode_levels(tex_rgba([texel], TEX_B8G8R8A8_UNORM))[0][0, 0]
    srgb = rt.decode_levels(tex_rgba([texel], TEX_B8G8R8A8_UNORM_SRGB))[0][0, 0]
    r8 = rt.decode_levels(rt.texture_dict([np.array([[77]], np.uint8)], TEX_R8_UNORM))[0][0, 0]
    u, s = rt.unorm_table(), rt.srgb_table()
    assert list(rgba) == [u[10], u[20], u[30]]
    assert list(bgra) == [u[30], u[20], u[10]]
    assert list(srgb) == [s[30], s[20], s[10]]
    assert list(r8) == [u[77], 0.0, 0.0]


def test_flat_normal_map_gives_the_geometric_normal(orc):
    """The restatement's textured resolve with a flat normal map ((128, 128, 255): ts ~ (0, 0, 1)) on a tilted quad with a random
    tangent: B is the geometric normal's code (within one step; 128 / 255 * 2 - 1 is 1 / 255, not 0), and a map of (255, 128, 128)
    (ts ~ +t) gives the tangent's code, (128, 255, 128) n x t's: the frame's axes in the restatement's own code."""
    from direct12pbrrenderer_amd.structs import Tile
    w, h = 48, 32
    cam = scene.Camera.reference_default(w, h)
    g = scene.make_global(cam, w, h)
    rot = scene.model_matrix((0.0, 0.0, 0.0), (20.0, -35.0, 10.0), (1.0, 1.0, 1.0)).astype(np.float64)
    inv_view = np.array(g.InvView[:], np.float64).reshape(4, 4)
    model = (inv_view @ np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 6], [0, 0, 0, 1]], np.float64) @ rot).astype(f32)
    quad = scene.quad_grid(1, 1, size=(30.0, 30.0))
    t = np.array([0.6, 0.8, 0.0])
    mesh = scene.Mesh(quad.vertices["position"], quad.vertices["normal"], quad.indices, tangents=np.broadcast_to(t, (4, 3)),
                      uvs=quad.vertices["position"][:, :2])
    R = model[:3, :3].astype(np.float64)
    n_w = R @ np.array([0.0, 0.0, -1.0])
    t_w = R @ t
    b_w = np.cross(n_w, t_w)
    for rgb, axis in (((128, 128, 255), n_w), ((255, 128, 128), t_w), ((128, 255, 128), b_w)):
        tex = rt.texture_dict([np.broadcast_to(np.array([*rgb, 255], np.uint8), (4, 4, 4)).copy()], TEX_R8G8B8A8_UNORM)
        ms = scene.MeshScene()
        ms.add(mesh, model, maps={"normal": 0})
        v, i, d = ms.arrays()
        got = rt.raster_textured(g, Tile(0, 0, w, h, w, h), v, i, d, ms.maps(), [tex], orc)
        cov = got["stencil"] > 0
        assert cov.mean() > 0.3
        m1 = np.zeros((1, 1, 4), f32)
        m1[0, 0, :3] = axis
        _, want, _ = orc.gbuffer_encode(np.zeros((1, 1, 4), f32), m1, np.zeros((1, 1, 4), f32))
        code = np.frombuffer(want.tobytes(), np.uint8)[:2].astype(np.int32)
        B = got["B"].view(np.uint8).reshape(h, w, 4)[..., :2].astype(np.int32)
        assert np.abs(B[cov] - code).max() <= 1, (rgb, np.abs(B[cov] - code).max())


def test_fixture_shape_and_formats():
    """tests/golden/textured_models.npz (make_textured_models.py): the four textured models with meshes, world matrices, material
    defaults and all five maps; every chain in its stored format from 32 x 32 down; the revolver listed as missing."""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "textured_models.npz"))
    assert sorted(str(n) for n in fx["name"]) == ["barrel", "rock", "suitcase", "tile"]
    assert [str(n) for n in fx["missing"]] == ["revolver"]
    assert [str(k) for k in fx["maps"]] == list(DRAW_MAPS_DTYPE.names)
    for n in fx["name"]:
        v, idx = fx[f"{n}_vertices"], fx[f"{n}_indices"]
        assert v.dtype == f32 and v.shape[1] == 14 and len(idx) % 3 == 0 and idx.max() < len(v)
        assert fx[f"{n}_world"].shape == (4, 4) and fx[f"{n}_use"].all()
        assert np.array_equal(fx[f"{n}_material"], f32([1, 1, 1, 0, 1, 0]))       # IPipeline.h:71 defaults
        for k in fx["maps"]:
            w0, h0, mips0, fmt, w, h, mips = (int(x) for x in fx[f"{n}_{k}_info"])
            assert fmt in (TEX_R8G8B8A8_UNORM, TEX_B8G8R8A8_UNORM, TEX_B8G8R8A8_UNORM_SRGB, TEX_R8_UNORM)
            assert (w0, h0, mips0) == ((1024, 1024, 11) if n == "barrel" else (2048, 2048, 12))
            assert (w, h) == (32, 32) and w0 >> (mips0 - mips) == w
            texel = 1 if fmt == TEX_R8_UNORM else 4
            assert len(fx[f"{n}_{k}_texels"]) == sum((w >> l) * (h >> l) for l in range(mips)) * texel
        if n == "barrel":
            assert all(int(fx[f"{n}_{k}_info"][3]) == TEX_B8G8R8A8_UNORM_SRGB for k in fx["maps"])
    ms = scene.MeshScene()
    texs, names = scene.add_textured_models(ms, fx)
    assert len(texs) == 20 and len(ms.maps()) == 4 and (ms.maps().view(np.uint32) < 20).all()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "textured_models.npz")) <= 512 * 1024


def test_abi_layouts_match_the_header():
    src = open(os.path.join(ROOT, "include", "pbr_hip.h")).read()
    assert C.sizeof(Texture2D) == 24 and Texture2D.width.offset == 8 and Texture2D.format.offset == 20
    assert DRAW_MAPS_DTYPE.itemsize == 20 and DRAW_MAPS_DTYPE.names == ("albedo", "normal", "roughness", "metallic", "ao")
    for name, val in (("PBR_NO_MAP", NO_MAP), ("PBR_RASTER_MAX_TEXTURES", structs.RASTER_MAX_TEXTURES),
                      ("PBR_TEX_MAX_SIZE", structs.TEX_MAX_SIZE), ("PBR_TEX_R8G8B8A8_UNORM", TEX_R8G8B8A8_UNORM),
                      ("PBR_TEX_B8G8R8A8_UNORM", TEX_B8G8R8A8_UNORM), ("PBR_TEX_B8G8R8A8_UNORM_SRGB", TEX_B8G8R8A8_UNORM_SRGB),
                      ("PBR_TEX_R8_UNORM", TEX_R8_UNORM)):
        m = re.search(r"#define %s\s+(0x[0-9a-fA-F]+|\d+)u" % name, src)
        assert m and int(m.group(1), 0) == val, name
    fields = re.search(r"typedef struct pbr_draw_maps \{(.*?)\} pbr_draw_maps;", src, re.S).group(1)
    assert re.findall(r"\w+", fields.split(";")[0])[1:] == list(DRAW_MAPS_DTYPE.names)


def test_mip_chain_and_scene_maps():
    lv = scene.mip_chain(np.arange(8 * 6 * 4, dtype=np.uint8).reshape(6, 8, 4))
    assert [l.shape for l in lv] == [(6, 8, 4), (3, 4, 4), (1, 2, 4)]
    a = lv[0].astype(np.uint32)
    assert lv[1][0, 0, 0] == (a[0, 0, 0] + a[0, 1, 0] + a[1, 0, 0] + a[1, 1, 0] + 2) >> 2
    assert len(scene.pack_chain(lv)) == (48 + 12 + 2) * 4
    ms = scene.MeshScene()
    k = ms.add(scene.uv_sphere(4, 6), np.eye(4), maps={"normal": 2, "ao": 0})
    ms.add(k, np.eye(4))
    m = ms.maps()
    assert m.dtype == DRAW_MAPS_DTYPE and len(m) == 2
    assert tuple(int(x) for x in m[0]) == (NO_MAP, 2, NO_MAP, NO_MAP, 0) and all(int(x) == NO_MAP for x in m[1])
