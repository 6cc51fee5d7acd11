#!/usr/bin/env python3
"""Times pbr_gbuffer_raster with bounds against the unculled calls and writes
profiles/raster_cull_ms.txt.

Each round is a fresh process.  In a round every scene is warmed up for both calls, then blocks of `--iters` culled calls and
`--iters` unculled calls alternate (`--blocks` of each, HIP events around a block); the round's figure is the median block.  The
file reports, per scene, the median over the rounds and the spread (min .. max) of the rounds for both calls, and the share of the
triangles the cull removed (pbr_cull_stats).

Scenes: the fixture scenes (the 33 constant models of sphere_grid.npz; with the four textured models of textured_models.npz through
the textured calls) from the reference camera at 1440x960 and 3840x2160, the same with the camera yawed until about half of the draws
it kept have left the view, each tile of a 2 x 2 grid of the 4K frame, and instanced spheres (24576 draws of one small mesh): all around the
camera, and all in view (nothing culled: the feature's price).
Usage: python tools/raster_cull_ms.py [--rounds 3] [--iters 20] [--blocks 5] [--out profiles/raster_cull_ms.txt]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import raster_cull_ref as rc  # noqa: E402
from direct12pbrrenderer_amd import scene  # noqa: E402
from direct12pbrrenderer_amd.structs import Tile  # noqa: E402

N_INSTANCES = 24576


def camera(w, h, yaw=0.0):
    cam = scene.Camera.reference_default(w, h)
    if yaw:
        cam.rotate(0.0, yaw, 0.0)
    return scene.make_global(cam, w, h)


def half_yaw(v, i, d):
    """the yaw (a multiple of 0.05 rad) at which about half of the draws the reference camera keeps have left the view, found with
    the rule on the CPU (the reference camera stands close to the sphere grid and keeps about half of the scene's draws itself)"""
    b = scene.draw_bounds(v, i, d)

    def share(yaw):
        g = camera(1440, 960, yaw)
        return rc.cull(g.Projection[:], g.View[:], (0, 0, 1440, 960, 1440, 960), d, b).mean()
    target = share(0.0) + 0.5 * (1.0 - share(0.0))
    return min((abs(share(float(y)) - target), float(y)) for y in np.arange(0.05, 3.15, 0.05))[1]


def instanced(around):
    """N_INSTANCES draws of one small sphere: on a shell of directions all around the reference camera (most leave the view), or
    on a grid that fills the view (none does)"""
    ms = scene.MeshScene()
    k = ms.add_mesh(scene.uv_sphere(6, 8))
    eye = np.array([0.0, 3.0, 10.0])
    rng = np.random.default_rng(1)
    n = N_INSTANCES
    if around:
        dirs = rng.normal(size=(n, 3))
        pos = eye + dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * rng.uniform(20.0, 60.0, (n, 1))
    else:   # the reference camera looks down -z: a grid 40 in front of it, inside a 1.5 : 1 frame of 60 degrees
        side = int(np.ceil(np.sqrt(n)))
        gx, gy = np.meshgrid(np.linspace(-0.9, 0.9, side), np.linspace(-0.9, 0.9, side))
        th = np.tan(0.333 * np.pi / 2)
        pos = eye + np.stack([gx.ravel()[:n] * 40 * th * 1.5, gy.ravel()[:n] * 40 * th, np.full(n, -40.0)], axis=1)
    for p in pos:
        ms.add(k, scene.model_matrix(p, (0, 0, 0), (0.12, 0.12, 0.12)))
    return ms.arrays()


def rows():
    """(label, w, h, tile rectangle or None, yaw, kind)"""
    out = []
    for kind, label in (("grid", "33 constant models"), ("tex", "33 models + 4 textured")):
        for w, h in ((1440, 960), (3840, 2160)):
            out.append((f"{label}, reference camera", w, h, None, 0.0, kind))
            out.append((f"{label}, yawed (half of the kept)", w, h, None, "half", kind))
    for ty in range(2):
        for tx in range(2):
            out.append((f"33 constant models, tile {tx},{ty} of 2x2", 3840, 2160, (tx * 1920, ty * 1080, 1920, 1080), 0.0, "grid"))
    out.append((f"{N_INSTANCES} spheres all around", 1440, 960, None, 0.0, "around"))
    out.append((f"{N_INSTANCES} spheres all in view", 1440, 960, None, 0.0, "inview"))
    return out


def child(iters, blocks):
    import torch
    from direct12pbrrenderer_amd.api import PbrContext
    assert torch.cuda.is_available(), "raster_cull_ms.py needs the GPU"
    ctx = PbrContext(0)
    fx = np.load(os.path.join(ROOT, "tests", "golden", "sphere_grid.npz"))
    fxt = np.load(os.path.join(ROOT, "tests", "golden", "textured_models.npz"))
    scenes = {}

    def load(kind):
        if kind in scenes:
            return scenes[kind]
        maps = pairs = None
        if kind == "grid":
            (v, i, d), _ = scene.reference_models(fx)
        elif kind == "tex":
            ms = scene.MeshScene()
            scene.reference_models(fx, ms)
            texs, _ = scene.add_textured_models(ms, fxt)
            v, i, d = ms.arrays()
            maps, pairs = ms.maps(), scene.import_texture_table(ctx, texs)
        else:
            v, i, d = instanced(kind == "around")
        n = int((d["index_count"] // 3).sum())
        dev = (ctx.upload(v), len(v), ctx.upload(i), len(i), ctx.upload(d), len(d), n)
        bounds = ctx.draw_bounds(*dev[:6])
        scenes[kind] = dict(host=(v, i, d), dev=dev, bounds=bounds, maps=None if maps is None else ctx.upload(maps), pairs=pairs,
                            yaw=half_yaw(v, i, d) if kind in ("grid", "tex") else 0.0)
        return scenes[kind]

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    result = []
    for label, w, h, rect, yaw, kind in rows():
        s = load(kind)
        yaw = s["yaw"] if yaw == "half" else yaw
        g = camera(w, h, yaw)
        tile = Tile(*(rect or (0, 0, w, h)), w, h)
        n = s["dev"][6]
        textured = s["maps"] is not None
        planes = [ctx.zeros((tile.h, tile.w), k) for k in (torch.int32, torch.int32, torch.int32, torch.float32, torch.uint8)]
        scratch = (ctx.alloc_textured_raster_scratch if textured else ctx.alloc_raster_scratch)(tile.w, tile.h, n)
        stats = ctx.alloc_cull_stats()
        tex = (s["maps"], [p[1] for p in s["pairs"]]) if textured else ()
        plain = ctx.gbuffer_raster_textured if textured else ctx.gbuffer_raster
        culled = ctx.gbuffer_raster_textured_culled if textured else ctx.gbuffer_raster_culled

        def run_plain():
            plain(g, tile, *s["dev"], *planes, tile.w, scratch, *tex)

        def run_culled():
            culled(g, tile, *s["dev"], *planes, tile.w, scratch, *tex, s["bounds"], stats)
        for _ in range(3):
            run_plain()
            run_culled()
        torch.cuda.synchronize()
        st = ctx.read_cull_stats(stats)
        tc, tp = [], []
        for _ in range(blocks):
            tc.append(block(run_culled))
            tp.append(block(run_plain))
        result.append(dict(label=label, size=f"{w}x{h}", draws=s["dev"][5], triangles=n, draws_culled=st.draws_culled,
                           tri_share=st.triangles_culled / max(n, 1), plain=float(np.median(tp)), culled=float(np.median(tc)),
                           yaw=yaw))
        del planes, scratch
        torch.cuda.empty_cache()
    name = torch.cuda.get_device_name(0)
    ctx.close()
    print("RESULT " + json.dumps(dict(device=name, rows=result)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_cull_ms.txt"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.iters, a.blocks)
    rounds = []
    for r in range(a.rounds):   # a fresh process per round
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(a.iters), "--blocks", str(a.blocks)],
                           stdout=subprocess.PIPE, text=True, timeout=900)
        if p.returncode != 0:
            raise SystemExit(f"round {r} failed with status {p.returncode}")
        rounds.append(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
        print(f"round {r} done", flush=True)
    lines = [f"pbr_gbuffer_raster[_textured]_culled against the unculled call, {rounds[0]['device']}, HIP events; {a.rounds} rounds (fresh "
             f"processes), per round the median of {a.blocks} blocks of {a.iters} calls, culled and unculled blocks alternating; "
             "ms per call: median over the rounds [min .. max of the rounds]",
             f"{'scene':<44}{'size':>10}{'draws':>7}{'culled':>7}{'triangles':>10}{'tri culled':>11}  {'unculled ms':<28}{'culled ms':<28}"
             f"{'diff':>9}  verdict"]
    for k, row in enumerate(rounds[0]["rows"]):
        tp = [r["rows"][k]["plain"] for r in rounds]
        tc = [r["rows"][k]["culled"] for r in rounds]
        mp, mc = float(np.median(tp)), float(np.median(tc))
        spread = max(tp) - min(tp)
        verdict = "within the unculled spread" if abs(mc - mp) <= spread else ("faster" if mc < mp else "slower: the price")
        lines.append(f"{row['label']:<44}{row['size']:>10}{row['draws']:>7}{row['draws_culled']:>7}{row['triangles']:>10}"
                     f"{100 * row['tri_share']:>10.1f}%  {f'{mp:.4f} [{min(tp):.4f} .. {max(tp):.4f}]':<28}"
                     f"{f'{mc:.4f} [{min(tc):.4f} .. {max(tc):.4f}]':<28}{mc - mp:>+9.4f}  {verdict}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
