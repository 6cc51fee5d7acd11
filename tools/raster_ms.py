#!/usr/bin/env python3
"""Times pbr_gbuffer_raster alone (HIP events on the context's stream, after warm-up) and writes profiles/raster_ms.txt.

Scenes: the reference scene's 33 constant-material models (main.json's 5 x 5 sphere grid and 8 light impostors over
sphere_Mesh_data.bin, tests/golden/sphere_grid.npz) with the reference camera at 1440x960 and 3840x2160; two procedural ones:
~1 M small triangles (a jittered quad grid filling the view) and four screen-covering triangles.  Per scene: ms per call,
Mtri/s (input triangles), Gpixel/s (frame pixels), and the same frame's shade (pbr_deferred_shade, small IBL, the 8 lights) for
comparison.  Usage: python tools/raster_ms.py [--iters N] [--out profiles/raster_ms.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import common  # noqa: E402
from direct12pbrrenderer_amd import scene  # noqa: E402
from direct12pbrrenderer_amd.api import PbrContext  # noqa: E402
from direct12pbrrenderer_amd.pipeline import DeferredFrame, TileSpec  # noqa: E402
from direct12pbrrenderer_amd.structs import Tile  # noqa: E402
from oracle import binding as orc  # noqa: E402


def timed(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def small_triangles(g, cam, n_side):
    """~2 n_side^2 small triangles: a jittered grid filling the view at depth 8 (front-facing)"""
    th = np.tan(float(cam.fov) / 2.0)
    grid = scene.quad_grid(n_side, n_side, size=(2.0 * 8 * th * float(cam.ratio), 2.0 * 8 * th), jitter=0.3, seed=1)
    to_view = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 8], [0, 0, 0, 1]], dtype=np.float64)
    ms = scene.MeshScene()
    ms.add(grid, (np.array(g.InvView[:], np.float64).reshape(4, 4) @ to_view).astype(np.float32))
    return ms.arrays()


def covering(g, cam):
    """4 screen-covering triangles (two quads at depth 5 and 7)"""
    th = np.tan(float(cam.fov) / 2.0)
    ms = scene.MeshScene()
    for z in (7.0, 5.0):
        q = scene.quad_grid(1, 1, size=(2.2 * z * th * float(cam.ratio), 2.2 * z * th))
        to_view = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, z], [0, 0, 0, 1]], dtype=np.float64)
        ms.add(q, (np.array(g.InvView[:], np.float64).reshape(4, 4) @ to_view).astype(np.float32))
    return ms.arrays()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_ms.txt"))
    a = ap.parse_args()
    ctx = PbrContext(0)
    sky, env, lut, sh = common.small_ibl(orc)
    rec = common.reference_scene_lights()
    fx = np.load(os.path.join(ROOT, "tests", "golden", "sphere_grid.npz"))
    lights = np.concatenate([scene.make_lights(rec["translation"][j], rec["color"][j], rec["radius"][j], rec["intensity"][j])
                             for j in range(len(rec["radius"]))])
    lines = [f"pbr_gbuffer_raster, {torch.cuda.get_device_name(0)}, HIP events, {a.iters} calls after 5 warm-up calls; "
             "shade = pbr_deferred_shade of the same frame (8 lights, 16^2 env / 32^2 LUT)",
             f"{'scene':<30}{'size':>11}{'triangles':>11}{'raster ms':>11}{'Mtri/s':>9}{'Gpx/s':>8}{'shade ms':>10}{'covered':>9}"]
    for name, w, h, kind in [("reference scene, 33 models", 1440, 960, "grid"), ("reference scene, 33 models", 3840, 2160, "grid"),
                             ("procedural small triangles", 1440, 960, "small"), ("procedural screen-covering", 1440, 960, "cover"),
                             ("procedural screen-covering", 3840, 2160, "cover")]:
        cam = scene.Camera.reference_default(w, h)
        g = scene.make_global(cam, w, h, sh_pack=sh)
        if kind == "grid":
            (v, i, d), _ = scene.reference_models(fx)
        elif kind == "small":
            v, i, d = small_triangles(g, cam, 708)
        else:
            v, i, d = covering(g, cam)

        def dev_half(x):
            return ctx.upload(np.ascontiguousarray(x, dtype=np.float16).view(np.uint16)).view(torch.float16)
        fr = DeferredFrame(ctx, TileSpec(0, 0, w, h, w, h, 0), g, lights, dev_half(lut), lut.shape[0], dev_half(env),
                           common.ENV_SIZE, common.ENV_MIPS)
        fr.set_meshes(v, i, d)
        n = fr.mesh["max_triangles"]
        ms_r = timed(fr.rasterize, a.iters)
        fr.clustered()
        ms_s = timed(fr.shade, a.iters)
        cov = float((fr.gb["stencil"] > 0).float().mean())
        lines.append(f"{name:<30}{f'{w}x{h}':>11}{n:>11}{ms_r:>11.4f}{n / ms_r / 1e3:>9.1f}{w * h / ms_r / 1e6:>8.2f}{ms_s:>10.4f}{cov:>9.3f}")
        print(lines[-1], flush=True)
        del fr
        torch.cuda.empty_cache()
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
