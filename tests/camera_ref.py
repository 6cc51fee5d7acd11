"""The camera-dependent geometry of the frame in plain numpy float64, from the formulas (a pinhole camera looking along +z of its
view space, ndc.z in [0, 1], the 24 x 16 x 8 cluster grid with exponential depth slices, a cube map's face convention) and not from
the shaders' order of operations: the world position goes through inv(Projection @ View) of the constant buffer where the shader walks
CameraPos + InvView * camera_vec * z / Near, so a wrong InvView entry in a kernel (or in the fp32 CPU oracle) cannot cancel here."""
import numpy as np

CLUSTER_X, CLUSTER_Y, CLUSTER_Z, MAX_PER_CLUSTER = 24, 16, 8, 32


def _m(field):
    return np.array(field[:], dtype=np.float64).reshape(4, 4)


def _ndc(tile):
    """pixel-centre NDC x [w] and y [h] of a tile (y up)"""
    x = (tile.x0 + np.arange(tile.w) + 0.5) / tile.full_w
    y = (tile.y0 + np.arange(tile.h) + 0.5) / tile.full_h
    return 2.0 * x - 1.0, 1.0 - 2.0 * y


def _unproject(g, ndc_x, ndc_y, depth):
    inv = np.linalg.inv(_m(g.Projection) @ _m(g.View))
    depth = np.broadcast_to(np.asarray(depth, dtype=np.float64), (len(ndc_y), len(ndc_x)))
    clip = np.stack([np.broadcast_to(ndc_x[None, :], depth.shape), np.broadcast_to(ndc_y[:, None], depth.shape), depth, np.ones(depth.shape)], axis=-1)
    p = clip @ inv.T
    return p[..., :3] / p[..., 3:4]


def unproject(g, tile, depth):
    """world position [h, w, 3] of every pixel of the tile at its NDC depth [h, w]"""
    return _unproject(g, *_ndc(tile), depth)


def ray_dirs(g, tile):
    """unit world-space view ray [h, w, 3] through every pixel centre: from the near plane's point to the far plane's"""
    nx, ny = _ndc(tile)
    d = _unproject(g, nx, ny, 1.0) - _unproject(g, nx, ny, 0.0)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def cube_face_coords(d, size):
    """(face, x, y) of directions [..., 3] in synth.cube_directions' convention — texel (row i, column j) of a face has its centre at
    y = i + 0.5, x = j + 0.5 — faces +x -x +y -y +z -z with (u, v) = (-z, -y) (z, -y) (x, z) (x, -z) (x, -y) (-x, -y) over |major|"""
    d = np.asarray(d, dtype=np.float64)
    a = np.abs(d)
    axis = a.argmax(axis=-1)
    major = np.take_along_axis(d, axis[..., None], -1)[..., 0]
    face = 2 * axis + (major < 0)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    u = np.choose(face, [-z, z, x, x, x, -x]) / np.abs(major)
    v = np.choose(face, [-y, -y, z, -z, -y, -y]) / np.abs(major)
    return face, (u + 1.0) * 0.5 * size, (v + 1.0) * 0.5 * size


def cluster_boxes(g):
    """(min [3072, 3], max [3072, 3]): the view-space AABB of every cluster's frustum cell (its eight corners), cluster
    (tx, ty, z) at index z + 8 tx + 192 ty; slice z spans view depths Near (Far / Near)^(z / 8) .. ^((z + 1) / 8)"""
    near, far, tan_y = float(g.Near), float(g.Far), np.tan(float(g.Fov) / 2.0)
    tan_x = tan_y * float(g.Ratio)
    ty, tx, z = np.meshgrid(np.arange(CLUSTER_Y), np.arange(CLUSTER_X), np.arange(CLUSTER_Z), indexing="ij")
    corners = []
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                depth = near * (far / near) ** ((z + dz) / CLUSTER_Z)
                corners.append(np.stack([(2.0 * (tx + dx) / CLUSTER_X - 1.0) * tan_x * depth, (2.0 * (ty + dy) / CLUSTER_Y - 1.0) * tan_y * depth,
                                         depth], axis=-1))
    corners = np.stack(corners, axis=0).reshape(8, -1, 3)     # C order of (ty, tx, z) is the cluster index
    return corners.min(axis=0), corners.max(axis=0)


def cull(g, lights, boxes, margin):
    """(lists, undecided): per cluster the lights (ascending index) whose sphere of radius Radius * 1.814 * sqrt(Intensity) around the
    view-space position reaches into the box — d^2 < r^2, d the distance to the box — and whether any pair of the cluster has
    |d^2 - r^2| <= margin * r^2, i.e. could fall either way in float32.  boxes: (min, max) [3072, 3]."""
    mn, mx = (np.asarray(b, dtype=np.float64) for b in boxes)
    view = _m(g.View)
    p = np.asarray(lights["Position"], dtype=np.float64).reshape(-1, 3)
    pv = (view @ np.c_[p, np.ones(len(p))].T).T[:, :3]
    r2 = (lights["Radius"].astype(np.float64) * 1.814 * np.sqrt(lights["Intensity"].astype(np.float64))) ** 2
    d2 = np.zeros((len(mn), len(pv)))
    for k in range(3):
        c = np.clip(pv[None, :, k], mn[:, None, k], mx[:, None, k])
        d2 += (pv[None, :, k] - c) ** 2
    hit = d2 < r2[None, :]
    undecided = (np.abs(d2 - r2[None, :]) <= margin * r2[None, :]).any(axis=1)
    return [np.flatnonzero(h) for h in hit], undecided


def lists_of_table(table):
    """a cluster table's used LightIndex entries, per cluster"""
    return [table["LightIndex"][c][:n] for c, n in enumerate(np.clip(table["NumLights"], 0, MAX_PER_CLUSTER))]
