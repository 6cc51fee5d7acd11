"""Host-side mirrors of the reference's per-frame CPU logic that feeds the shading path.

* Camera            <- Engine/Include/Renderer/Camera.h:9-50, Engine/Source/Renderer/Camera.cpp:5-12
* projection_matrix1 <- Engine/Source/Utils/MathLib.cpp:35-68 (ndc.z in [0,1], left-handed)
* from_euler_angle  <- Engine/Include/Utils/MathLib.h:656-671
* quick_inverse     <- Engine/Include/Utils/MathLib.h:786-811
* make_global       <- RenderScheduler::ExecutePipeline, Engine/Source/Renderer/RenderScheduler.cpp:22-38
* attenuation presets / CaclAttenuationCoefficients <- Engine/Include/Renderer/Scene.h:126-142,
  Engine/Source/Renderer/Scene.cpp:132-165
* model_matrix      <- SceneObject::PostDeserialized, Engine/Source/Renderer/Scene.cpp:31-36
* Mesh / MeshScene  <- what DrawModel binds per draw (DeferredPipeline.cpp:138-185): vertex + index buffers and
  ConstantBufferInstance (gbuffer.hlsl:33-48), the input of pbr_gbuffer_raster

Everything is evaluated in float32 like the reference's Vector/Matrix classes.
"""
import ctypes as C
import math

import numpy as np

from .structs import AABB_DTYPE, DRAW_DTYPE, DRAW_MAPS_DTYPE, LIGHT_DTYPE, NO_MAP, VERTEX_DTYPE, Global, ShPack

f32 = np.float32
PI = f32(3.14159265359)


def projection_matrix1(fov, ratio, near_z, far_z):
    fov, ratio, near_z, far_z = f32(fov), f32(ratio), f32(near_z), f32(far_z)
    htan = f32(math.tan(float(fov * f32(0.5))))
    r = near_z * ratio * htan
    l = -r
    t = near_z * htan
    b = -t
    m = np.zeros((4, 4), dtype=f32)
    m[0, 0] = (f32(2) * near_z) / (r - l)
    m[0, 2] = (r + l) / (l - r)
    m[1, 1] = (f32(2) * near_z) / (t - b)
    m[1, 2] = (t + b) / (b - t)
    m[2, 2] = far_z / (far_z - near_z)
    m[2, 3] = (near_z * far_z) / (near_z - far_z)
    m[3, 2] = f32(1)
    return m


def from_euler_angle(yaw, pitch, roll):
    """Matrix3x3::FromEulerAngle(yaw, pitch, roll) — parameter NAMES as in MathLib.h:656."""
    ca, sa = f32(math.cos(yaw)), f32(math.sin(yaw))
    cb, sb = f32(math.cos(pitch)), f32(math.sin(pitch))
    cc, sc = f32(math.cos(roll)), f32(math.sin(roll))
    return np.array([
        [ca * cb, ca * sb * sc - sa * cc, ca * sb * cc + sa * sc],
        [sa * cb, sa * sb * sc + ca * cc, sa * sb * cc - ca * sc],
        [-sb, cb * sc, cb * cc]], dtype=f32)


def quick_inverse(m):
    """Matrix4x4::QuickInverse: inverse of a rotation*scale + translation transform."""
    scale = np.sqrt((m[:3, :3].astype(f32) ** 2).sum(axis=0, dtype=f32)).astype(f32)
    rot = (m[:3, :3] / scale[None, :]).astype(f32).T
    inv_scale = (f32(1) / scale).astype(f32)
    inv_m = (rot * inv_scale[None, :]).astype(f32)
    tr = m[:3, 3]
    inv_t = np.array([(inv_m[i, 0] * tr[0] + inv_m[i, 1] * tr[1]) + inv_m[i, 2] * tr[2] for i in range(3)], dtype=f32)
    out = np.zeros((4, 4), dtype=f32)
    out[:3, :3] = inv_m
    out[:3, 3] = -inv_t
    out[3, 3] = f32(1)
    return out


class Camera:
    """Camera.h:9-50.  The transform is view-space -> world-space (row-major, M*v)."""

    def __init__(self, fov, width, height, near_plane, far_plane):
        self.fov = f32(fov)
        self.ratio = f32(width) / f32(height)
        self.near = f32(near_plane)
        self.far = f32(far_plane)
        self.roll = self.yaw = self.pitch = 0.0
        self.transform = np.eye(4, dtype=f32)

    def move(self, delta):
        self.transform[:3, 3] += np.asarray(delta, dtype=f32)

    def rotate(self, roll, yaw, pitch):
        # Camera.cpp:5-12: SetRotation(FromEulerAngle(mRoll, mYaw, mPitch)) — the arguments land on
        # FromEulerAngle's (yaw, pitch, roll) parameters in that order.
        self.roll += roll
        self.yaw += yaw
        self.pitch += pitch
        scale = np.sqrt((self.transform[:3, :3] ** 2).sum(axis=0, dtype=f32)).astype(f32)
        self.transform[:3, :3] = from_euler_angle(self.roll, self.yaw, self.pitch) * scale[None, :]

    def world_matrix(self):
        return self.transform.copy()

    def local_space_matrix(self):
        return quick_inverse(self.transform)

    def projection_matrix(self):
        return projection_matrix1(self.fov, self.ratio, self.near, self.far)

    def translation(self):
        return self.transform[:3, 3].copy()

    @staticmethod
    def reference_default(width, height):
        """App.cpp:99-101: Fov 0.333*PI, Near 0.1, Far 1000, Move(0,3,10), Rotate(0, PI, 0)."""
        cam = Camera(f32(0.333) * PI, width, height, 0.1, 1000.0)
        cam.move((0.0, 3.0, 10.0))
        cam.rotate(0.0, float(PI), 0.0)
        return cam


def make_global(camera, width, height, sh_pack=None, delta_time=1.0 / 60.0, time=0.0):
    """Fill ConstantBufferGlobal the way RenderScheduler::ExecutePipeline does (RenderScheduler.cpp:22-38)."""
    g = Global()
    if sh_pack is not None:
        arr = np.asarray(sh_pack, dtype=f32).reshape(28)
        C.memmove(C.byref(g.SkyBoxSH), arr.ctypes.data, 112)
    proj = camera.projection_matrix()
    mats = {
        "InvView": camera.world_matrix(),
        "View": camera.local_space_matrix(),
        "Projection": proj,
        "InvProjection": np.linalg.inv(proj.astype(np.float64)).astype(f32),
    }
    for name, m in mats.items():
        getattr(g, name)[:] = [float(v) for v in np.ascontiguousarray(m, dtype=f32).reshape(16)]
    g.CameraPos[:] = [float(v) for v in camera.translation()]
    g.Ratio = float(camera.ratio)
    g.Resolution[:] = [float(width), float(height)]
    g.Near = float(camera.near)
    g.Far = float(camera.far)
    g.Fov = float(camera.fov)
    g.DeltaTime = float(f32(delta_time))
    g.Time = float(f32(time))
    return g


# Scene.h:126-142
ATTENUATION_PRESETS = [
    (0.1, 1.0, 45.0, 7500.0), (1.0, 1.0, 4.5, 75.0), (7.0, 1.0, 0.7, 1.8), (13.0, 1.0, 0.35, 0.44),
    (20.0, 1.0, 0.22, 0.2), (32.0, 1.0, 0.14, 0.07), (50.0, 1.0, 0.09, 0.032), (65.0, 1.0, 0.07, 0.017),
    (100.0, 1.0, 0.045, 0.0075), (160.0, 1.0, 0.027, 0.0028), (200.0, 1.0, 0.022, 0.0019),
    (325.0, 1.0, 0.014, 0.0007), (600.0, 1.0, 0.007, 0.0002),
]


def attenuation_coefficients(radius):
    """SceneLight::CaclAttenuationCoefficients (Scene.cpp:132-165).

    The interpolation branch tests `radius >= P[i].Radius && radius <= P[i].Radius` on the SAME
    preset, so it only fires on exact equality (k = 0): the function is a step function (quirk Q18).
    Returns (Radius, C0, C1, C2).
    """
    radius = float(f32(radius))
    for i in range(len(ATTENUATION_PRESETS) - 1):
        lower = ATTENUATION_PRESETS[i]
        if radius < float(f32(lower[0])):
            return (radius, lower[1], lower[2], lower[3])
        if radius == float(f32(lower[0])):
            return (radius, lower[1], lower[2], lower[3])   # k == 0 -> lower
    last = ATTENUATION_PRESETS[-1]
    return (last[0], last[1], last[2], last[3])


def make_lights(positions, colors, radius, intensity):
    """PointLight records as ClusteredPass::Execute uploads them (DeferredPipeline.cpp:225-250)."""
    positions = np.asarray(positions, dtype=f32).reshape(-1, 3)
    n = positions.shape[0]
    lights = np.zeros(n, dtype=LIGHT_DTYPE)
    lights["Position"] = positions
    lights["Color"] = np.asarray(colors, dtype=f32).reshape(-1, 3)
    lights["Intensity"] = f32(intensity)
    r, c0, c1, c2 = attenuation_coefficients(radius)
    lights["Radius"], lights["C0"], lights["C1"], lights["C2"] = f32(r), f32(c0), f32(c1), f32(c2)
    return lights


def sh_pack_struct(arr28):
    p = ShPack()
    a = np.asarray(arr28, dtype=f32).reshape(28)
    C.memmove(C.byref(p), a.ctypes.data, 112)
    return p


def scene_file_text(recs, extra_members=True):
    """A scene file in the reference serializer's shape (Serialization.h:180-236: base class under "@<Base>", Vector3 as {x, y, z})
    holding these light records (dict-like of arrays: name, translation, rotation, scale, color, radius, intensity) — what
    pbrh_load_scene_lights reads; generated input, not the reference's asset."""
    import json

    def v(a):
        return {"x": float(a[0]), "y": float(a[1]), "z": float(a[2])}
    lights = [{"@SceneObject": {"mName": str(recs["name"][i]), "mTranslation": v(recs["translation"][i]),
                                "mRotation": v(recs["rotation"][i]), "mScale": v(recs["scale"][i])},
               "mColor": v(recs["color"][i]), "mRadius": float(recs["radius"][i]), "mIntensity": float(recs["intensity"][i])}
              for i in range(len(recs["radius"]))]
    doc = {"@IResource": None, "mSceneLight": lights}
    if extra_members:   # members of the file the light path must skip over
        doc["mSceneModel"] = [{"@SceneObject": {"mName": "m\u00e9sh \"0\"", "mTranslation": v([0, 0, 0]), "mRotation": v([0, 90, 0]),
                                                "mScale": v([0.1, 0.1, 0.1])}, "mModelFilePath": "Asset/Model/x.json"}]
        doc["mSkyBoxPath"] = "Asset/SkyBox/none"
    return json.dumps(doc, indent=1)


DEG2RAD = PI / f32(180.0)


def model_matrix(translation, rotation_deg, scale):
    """SceneObject::PostDeserialized (Scene.cpp:31-36): FromEulerAngle(rotation in degrees) with its columns scaled by `scale`,
    plus the translation (the rule host/SceneFile.cpp applies to the scene file's lights)."""
    r = [float(f32(a) * DEG2RAD) for a in rotation_deg]
    m = np.eye(4, dtype=f32)
    m[:3, :3] = from_euler_angle(*r) * np.asarray(scale, dtype=f32)[None, :]
    m[:3, 3] = np.asarray(translation, dtype=f32)
    return m


# Matrix4x4::Inverse (Engine/Include/Utils/MathLib.h:813-940, the cofactor expansion of MESA's gluInvertMatrix), which the reference
# evaluates for every draw's InvModel (DeferredPipeline.cpp:173): entry k of the row-major result = its six signed triple
# products m[a] * m[b] * m[c], summed left to right in float32, times 1 / det.
_INV_TERMS = {
    0: ("+--++-", "5.10.15 5.11.14 9.6.15 9.7.14 13.6.11 13.7.10"), 1: ("-++--+", "1.10.15 1.11.14 9.2.15 9.3.14 13.2.11 13.3.10"),
    2: ("+--++-", "1.6.15 1.7.14 5.2.15 5.3.14 13.2.7 13.3.6"), 3: ("-++--+", "1.6.11 1.7.10 5.2.11 5.3.10 9.2.7 9.3.6"),
    4: ("-++--+", "4.10.15 4.11.14 8.6.15 8.7.14 12.6.11 12.7.10"), 5: ("+--++-", "0.10.15 0.11.14 8.2.15 8.3.14 12.2.11 12.3.10"),
    6: ("-++--+", "0.6.15 0.7.14 4.2.15 4.3.14 12.2.7 12.3.6"), 7: ("+--++-", "0.6.11 0.7.10 4.2.11 4.3.10 8.2.7 8.3.6"),
    8: ("+--++-", "4.9.15 4.11.13 8.5.15 8.7.13 12.5.11 12.7.9"), 9: ("-++--+", "0.9.15 0.11.13 8.1.15 8.3.13 12.1.11 12.3.9"),
    10: ("+--++-", "0.5.15 0.7.13 4.1.15 4.3.13 12.1.7 12.3.5"), 11: ("-++--+", "0.5.11 0.7.9 4.1.11 4.3.9 8.1.7 8.3.5"),
    12: ("-++--+", "4.9.14 4.10.13 8.5.14 8.6.13 12.5.10 12.6.9"), 13: ("+--++-", "0.9.14 0.10.13 8.1.14 8.2.13 12.1.10 12.2.9"),
    14: ("-++--+", "0.5.14 0.6.13 4.1.14 4.2.13 12.1.6 12.2.5"), 15: ("+--++-", "0.5.10 0.6.9 4.1.10 4.2.9 8.1.6 8.2.5"),
}


def inverse(m):
    """Matrix4x4::Inverse in float32 (the draw's InvModel): cofactors, det = m0 inv0 + m1 inv4 + m2 inv8 + m3 inv12, identity if
    det == 0, else inv * (1 / det)."""
    a = [f32(v) for v in np.asarray(m, dtype=f32).reshape(16)]
    inv = []
    for k in range(16):
        signs, terms = _INV_TERMS[k]
        acc = None
        for sg, t in zip(signs, terms.split()):
            i, j, l = (int(x) for x in t.split("."))
            p = (-a[i] if sg == "-" else a[i]) * a[j] * a[l] if acc is None else a[i] * a[j] * a[l]
            acc = p if acc is None else (acc + p if sg == "+" else acc - p)
        inv.append(acc)
    det = ((a[0] * inv[0] + a[1] * inv[4]) + a[2] * inv[8]) + a[3] * inv[12]
    if det == 0:
        return np.eye(4, dtype=f32)
    inv_det = f32(1.0) / det
    return np.array([v * inv_det for v in inv], dtype=f32).reshape(4, 4)


class Mesh:
    """One vertex buffer (structs.VERTEX_DTYPE: position, normal, tangent, colour, uv) and its uint32 triangle list."""

    def __init__(self, positions, normals, indices, tangents=None, uvs=None):
        positions = np.asarray(positions, dtype=f32).reshape(-1, 3)
        self.vertices = np.zeros(len(positions), dtype=VERTEX_DTYPE)
        self.vertices["position"] = positions
        self.vertices["normal"] = np.asarray(normals, dtype=f32).reshape(-1, 3)
        if tangents is not None:
            self.vertices["tangent"] = np.asarray(tangents, dtype=f32).reshape(-1, 3)
        if uvs is not None:
            self.vertices["uv"] = np.asarray(uvs, dtype=f32).reshape(-1, 2)
        self.indices = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)

    @property
    def n_triangles(self):
        return len(self.indices) // 3


def _orient(positions, tris, outward):
    """Triangles wound so that (b - a) x (c - a) points along outward(a, b, c): front-facing (clockwise on screen, the
    DefaultOpaque state) when seen from that side."""
    p = positions[tris]
    cr = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    flip = (cr * outward(p)).sum(axis=1) < 0
    tris = tris.copy()
    tris[flip, 1], tris[flip, 2] = tris[flip, 2], tris[flip, 1].copy()
    return tris


def uv_sphere(n_lat, n_lon, radius=1.0):
    """A UV sphere of radius `radius` around the origin: n_lat rings of n_lon quads (fans at the poles), vertex normals =
    the unit position, every triangle facing outwards."""
    th = np.linspace(0.0, np.pi, n_lat + 1)
    ph = np.linspace(0.0, 2.0 * np.pi, n_lon + 1)[:-1]
    dirs = np.stack([np.sin(th)[:, None] * np.cos(ph)[None, :], np.cos(th)[:, None] * np.ones_like(ph)[None, :],
                     np.sin(th)[:, None] * np.sin(ph)[None, :]], axis=-1).reshape(-1, 3)
    vid = np.arange((n_lat + 1) * n_lon).reshape(n_lat + 1, n_lon)
    tris = []
    for i in range(n_lat):
        for j in range(n_lon):
            a, b, c, d = vid[i, j], vid[i, (j + 1) % n_lon], vid[i + 1, (j + 1) % n_lon], vid[i + 1, j]
            if i != 0:
                tris.append((a, b, c))
            if i != n_lat - 1:
                tris.append((a, c, d))
    tris = _orient(dirs, np.array(tris, dtype=np.int64), lambda p: p.mean(axis=1))
    return Mesh(dirs * radius, dirs, tris)


def quad_grid(nx, ny, size=(2.0, 2.0), jitter=0.0, seed=0, normal_sign=1.0):
    """An nx x ny grid of quads in the z = 0 plane, centred on the origin, `size` wide and high; interior grid points moved
    by up to `jitter` of a cell (shared by the neighbouring quads: the mesh stays closed).  Triangles face -z (towards a viewer
    on the -z side looking along +z) with normal_sign 1, +z with -1; vertex normals (0, 0, -normal_sign)."""
    xs = (np.arange(nx + 1) / nx - 0.5) * size[0]
    ys = (np.arange(ny + 1) / ny - 0.5) * size[1]
    p = np.zeros((ny + 1, nx + 1, 3))
    p[..., 0], p[..., 1] = xs[None, :], ys[:, None]
    if jitter:
        rng = np.random.default_rng(seed)
        d = rng.uniform(-jitter, jitter, (ny - 1, nx - 1, 2))
        p[1:-1, 1:-1, 0] += d[..., 0] * size[0] / nx
        p[1:-1, 1:-1, 1] += d[..., 1] * size[1] / ny
    vid = np.arange((ny + 1) * (nx + 1)).reshape(ny + 1, nx + 1)
    a, b, c, d = vid[:-1, :-1], vid[:-1, 1:], vid[1:, 1:], vid[1:, :-1]
    tris = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], axis=2).reshape(-1, 3)
    face = np.array([0.0, 0.0, -float(normal_sign)])
    tris = _orient(p.reshape(-1, 3), tris, lambda q: np.broadcast_to(face, (len(q), 3)))
    return Mesh(p.reshape(-1, 3), np.broadcast_to(face, (len(p.reshape(-1, 3)), 3)), tris)


def _bound_key(a):
    """float32 -> an order-preserving uint32 key (-0 below +0), the order pbr_draw_bounds takes its min / max in"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return u ^ np.where(u >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def _bound_unkey(k):
    k = np.asarray(k, dtype=np.uint32)
    return (k ^ np.where(k >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)


def draw_bounds(vertices, indices, draws):
    """The host twin of pbr_draw_bounds: structs.AABB_DTYPE records, the exact min / max over the positions of each draw's triangles
    under the raster's guards (a range past the index buffer is skipped whole, a triangle with an index + base_vertex outside the
    vertex buffer is dropped; a NaN position takes no part); a draw without a valid triangle gets the inverted box (+FLT_MAX,
    -FLT_MAX), which the cull never culls."""
    vertices, indices, draws = np.asarray(vertices), np.asarray(indices, dtype=np.uint32), np.asarray(draws)
    out = np.zeros(len(draws), dtype=AABB_DTYPE)
    fmax = np.finfo(np.float32).max
    out["min"], out["max"] = fmax, -fmax
    pos = np.ascontiguousarray(vertices["position"], dtype=np.float32).reshape(-1, 3)
    for k, d in enumerate(draws):
        first, count, base = int(d["first_index"]), int(d["index_count"]), int(d["base_vertex"])
        if count < 3 or first + count > len(indices):
            continue
        vi = indices[first:first + 3 * (count // 3)].astype(np.int64).reshape(-1, 3) + base
        vi = vi[((vi >= 0) & (vi < len(pos))).all(axis=1)].reshape(-1)
        if not len(vi):
            continue
        p = pos[vi]
        key = _bound_key(p)
        ok = ~np.isnan(p)
        lo = np.where(ok, key, _bound_key(np.float32(fmax))).min(axis=0)
        hi = np.where(ok, key, _bound_key(np.float32(-fmax))).max(axis=0)
        out[k]["min"] = _bound_unkey(np.minimum(lo, _bound_key(np.float32(fmax))))
        out[k]["max"] = _bound_unkey(np.maximum(hi, _bound_key(np.float32(-fmax))))
    return out


def world_box(draws, bounds):
    """(min, max) float32: the union over the draws of the world box of each local box's eight corners through the draw's Model
    (float64, rounded outwards) — what the sun's light camera is fitted around (api.sun_fit).  A draw with the inverted box (no valid
    triangle) takes no part; None if no draw does."""
    lo, hi = None, None
    for d, b in zip(np.asarray(draws), np.asarray(bounds)):
        mn, mx = b["min"].astype(np.float64), b["max"].astype(np.float64)
        if (mn > mx).any():
            continue
        m = np.asarray(d["Model"], dtype=np.float64).reshape(4, 4)
        c = np.array([[(mx if i & 1 else mn)[0], (mx if i & 2 else mn)[1], (mx if i & 4 else mn)[2]] for i in range(8)])
        # sums left to right, as the C++ host's SunShadowPass::WorldBox forms them: the two give the same box to the bit
        w = np.stack([((m[r, 0] * c[:, 0] + m[r, 1] * c[:, 1]) + m[r, 2] * c[:, 2]) + m[r, 3] for r in range(3)], axis=1)
        lo = w.min(axis=0) if lo is None else np.minimum(lo, w.min(axis=0))
        hi = w.max(axis=0) if hi is None else np.maximum(hi, w.max(axis=0))
    if lo is None:
        return None
    return (np.nextafter(lo.astype(f32), f32(-np.inf)), np.nextafter(hi.astype(f32), f32(np.inf)))


class MeshScene:
    """Draws over shared buffers: add(mesh, model, albedo, emission, roughness, metallic) appends a mesh (or draws one added
    before again: instance=index) and one pbr_draw; arrays() -> (vertices, indices, draws), the input of pbr_gbuffer_raster."""

    def __init__(self):
        self._verts, self._idx, self._draws, self._ranges, self._maps = [], [], [], [], []
        self._nv = self._ni = 0

    def add_mesh(self, mesh):
        self._ranges.append((self._ni, len(mesh.indices), self._nv))
        self._verts.append(mesh.vertices)
        self._idx.append(mesh.indices)
        self._nv += len(mesh.vertices)
        self._ni += len(mesh.indices)
        return len(self._ranges) - 1

    def add(self, mesh, model, albedo=(1.0, 1.0, 1.0), emission=0.0, roughness=0.5, metallic=0.0, maps=None):
        """maps: {"albedo" | "normal" | "roughness" | "metallic" | "ao": texture index} (the Use*Map flags; a map left out takes
        the constant branch) -> the draw's record of maps()"""
        k = mesh if isinstance(mesh, int) else self.add_mesh(mesh)
        m = np.full((), NO_MAP, dtype=DRAW_MAPS_DTYPE)
        for name, t in (maps or {}).items():
            m[name] = t
        self._maps.append(m)
        first, count, base = self._ranges[k]
        d = np.zeros((), dtype=DRAW_DTYPE)
        d["Model"] = np.asarray(model, dtype=f32).reshape(16)
        d["InvModel"] = inverse(np.asarray(model, dtype=f32).reshape(4, 4)).reshape(16)
        d["Albedo"], d["Emission"], d["Roughness"], d["Metallic"] = albedo, emission, roughness, metallic
        d["first_index"], d["index_count"], d["base_vertex"] = first, count, base
        self._draws.append(d)
        return k

    def arrays(self):
        return (np.concatenate(self._verts) if self._verts else np.zeros(0, VERTEX_DTYPE),
                np.concatenate(self._idx).astype(np.uint32) if self._idx else np.zeros(0, np.uint32),
                np.array(self._draws, dtype=DRAW_DTYPE))

    def bounds(self):
        """the draws' local boxes (structs.AABB_DTYPE), parallel to arrays()[2]: draw_bounds of arrays(), the host twin of
        pbr_draw_bounds"""
        return draw_bounds(*self.arrays())

    def maps(self):
        """the draws' pbr_draw_maps records (structs.DRAW_MAPS_DTYPE), parallel to arrays()[2]"""
        return np.array(self._maps, dtype=DRAW_MAPS_DTYPE)


def mip_chain(level0, mip_levels=None):
    """A synthetic texture's mip chain: level0 (uint8 [h, w] or [h, w, channels]) and each next level the 2 x 2 box average of the
    one above ((a + b + c + d + 2) >> 2 on the stored bytes; an odd last row / column is dropped), down to mip_levels levels (all
    of them by default: floor(log2(min(w, h))) + 1).  The chain is input data: any chain is sampled as given."""
    lv = [np.ascontiguousarray(level0, dtype=np.uint8)]
    h, w = lv[0].shape[:2]
    n = int(np.floor(np.log2(min(w, h)))) + 1 if mip_levels is None else int(mip_levels)
    for i in range(1, n):
        a = lv[-1].astype(np.uint32)
        hh, ww = h >> i, w >> i
        a = a[:2 * hh, :2 * ww]
        s = a[0::2, 0::2] + a[1::2, 0::2] + a[0::2, 1::2] + a[1::2, 1::2]
        lv.append(((s + 2) >> 2).astype(np.uint8))
    return lv


def pack_chain(levels):
    """mip levels -> the bytes of the reference's layout (levels concatenated from level 0, rows tightly packed)"""
    return np.concatenate([np.ascontiguousarray(l).reshape(-1) for l in levels])

def reference_models(fx, ms=None):
    """The constant-material models of the reference's scene (Asset/Scene/main.json) from the fixture written by
    tests/golden/make_sphere_grid.py (fx: the loaded npz): one shared mesh (sphere_Mesh_data.bin) and one draw per model, in file
    order, appended to ms (a new MeshScene by default).  Returns ((vertices, indices, draws), names)."""
    verts = np.zeros(len(fx["vertices"]), dtype=VERTEX_DTYPE)
    verts.view(np.float32).reshape(-1, 14)[:] = fx["vertices"]
    ms = MeshScene() if ms is None else ms
    mesh = Mesh(verts["position"], verts["normal"], fx["indices"])
    mesh.vertices = verts
    k = ms.add_mesh(mesh)
    for world, mat in zip(fx["world"], fx["material"]):
        ms.add(k, world, albedo=tuple(mat[:3]), emission=mat[3], roughness=mat[4], metallic=mat[5])
    return ms.arrays(), [str(n) for n in fx["name"]]


def add_textured_models(ms, fx):
    """The textured models of the reference's scene from the fixture written by tests/golden/make_textured_models.py (fx: the
    loaded npz) appended to MeshScene ms: one mesh per model, one draw per sub-mesh with the model's world matrix, material
    constants and maps.  Returns (textures, names): textures in table order as dicts of the chain kept in the fixture (levels:
    uint8 arrays in the stored format, width, height, mips, format), which the draws' map indices point into."""
    textures, names = [], [str(n) for n in fx["name"]]
    for n in names:
        verts = np.zeros(len(fx[f"{n}_vertices"]), dtype=VERTEX_DTYPE)
        verts.view(np.float32).reshape(-1, 14)[:] = fx[f"{n}_vertices"]
        mesh = Mesh(verts["position"], verts["normal"], fx[f"{n}_indices"])
        mesh.vertices = verts
        mat = fx[f"{n}_material"]
        maps = {}
        for k in fx["maps"]:
            key = f"{n}_{k}_texels"
            if key not in fx.files:
                continue
            w0, h0, _, fmt, w, h, mips = (int(x) for x in fx[f"{n}_{k}_info"])
            ch = 1 if fmt == 61 else 4
            data, levels, o = fx[key], [], 0
            for l in range(mips):
                sz = (w >> l) * (h >> l) * ch
                lv = data[o:o + sz].reshape(h >> l, w >> l, ch)
                levels.append(lv[..., 0] if ch == 1 else lv)
                o += sz
            maps[str(k)] = len(textures)
            textures.append({"levels": levels, "width": w, "height": h, "mips": mips, "format": fmt})
        subs = fx[f"{n}_submeshes"]
        k = ms.add_mesh(mesh)
        first, _, base = ms._ranges[k]
        for start, count in subs:
            ms._ranges.append((first + int(start), int(count), base))
            ms.add(len(ms._ranges) - 1, fx[f"{n}_world"], albedo=tuple(mat[:3]), emission=mat[3], roughness=mat[4], metallic=mat[5],
                   maps=maps)
    return textures, names


def import_texture_table(ctx, textures, bc1=False):
    """add_textured_models' table brought in through PbrContext.import_texture: each texture's level 0 goes to the device and its
    chain (as many levels as the table's entry has) is made there by pbr_texture2d_gen_mips and, with bc1=True, compressed by
    pbr_bc1_encode.  Returns the (device tensor, Texture2D) pairs in table order, as DeferredFrame.set_meshes(..., textures=) takes
    them.  The levels the table holds below level 0 are not used: the chain is mip_chain's of its level 0."""
    return [ctx.import_texture(t["levels"][0], t["format"], mip_levels=t["mips"], bc1=bc1) for t in textures]


def bc1_texture_table(fxb):
    """The textured models' maps as BC1 chains from the fixture written by tests/golden/make_textured_models_bc1.py (fxb: the
    loaded npz), in add_textured_models' table order (model by model, the maps in `maps` order), so that the draws' map indices of
    add_textured_models point into it.  Returns dicts of the kept chain (from the 128 x 128 level down): blocks (uint8, the BC1
    payload: PbrContext.upload_texture(blocks, width, height, mips, format | structs.TEX_BC1_BLOCKS)), width, height, mips and
    the stored format."""
    table = []
    for n in (str(x) for x in fxb["name"]):
        for k in (str(x) for x in fxb["maps"]):
            if f"{n}_{k}_blocks" not in fxb.files:
                continue
            _, _, _, fmt, w, h, mips = (int(x) for x in fxb[f"{n}_{k}_info"])
            table.append({"blocks": fxb[f"{n}_{k}_blocks"], "width": w, "height": h, "mips": mips, "format": fmt})
    return table
