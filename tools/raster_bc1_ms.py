#!/usr/bin/env python3
"""Times pbr_gbuffer_raster with maps with BC1-resident textures against the same textures decoded by pbr_bc1_decode (HIP events on
the context's stream, after warm-up) and writes profiles/raster_bc1_ms.txt.

Scene and camera: those of tools/raster_tex_ms.py (the reference scene's 33 constant-material models plus barrel, rock, suitcase
and tile from the fixtures).  Textures: seeded random BC1 blocks at each map's original size, level count and stored format
(barrel 1024^2 x 11 levels, the others 2048^2 x 12): any 8 bytes are a valid block.  Rows per size (1440x960, 3840x2160):
  decoded-resident   the chains pbr_bc1_decode produces from the blocks (what the reference holds after its load-time decode)
  BC1-resident       the same blocks, sampled in place
Both rows sample identical texel values; their five planes are compared before anything is timed.  Columns: raster ms, the bytes of
the resident texture table, and the one-off pbr_bc1_decode time of the whole table (one pass over the 20 chains, after a warm-up pass).

--parent-runs / --this-runs: output files of tools/raster_tex_ms.py (--out) from alternating runs of the parent commit's and this
commit's tree in one session; their "constant-only" and "textured" rows, the parent's spread against itself (max - min over its
runs) and the difference of the medians are appended: the existing path's regression check.
Usage: python tools/raster_bc1_ms.py [--iters N] [--out profiles/raster_bc1_ms.txt] [--parent-runs F... --this-runs F...]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def tex_ms_rows(path):
    """{(row, size): raster ms} of one raster_tex_ms.py output file"""
    rows = {}
    for line in open(path):
        f = line.split()
        if len(f) == 7 and f[0] in ("constant-only", "textured"):
            rows[(f[0], f[1])] = float(f[3])
    return rows


def regression_lines(parent_files, this_files):
    parent, this = [tex_ms_rows(p) for p in parent_files], [tex_ms_rows(p) for p in this_files]
    lines = ["", f"existing path, tools/raster_tex_ms.py of the parent commit and of this commit run alternately in one session "
             f"({len(parent)} + {len(this)} runs), raster ms:",
             f"{'row':<16}{'size':>11}  {'parent runs':<34}{'this commit runs':<34}{'parent max-min':>15}{'median diff':>13}  verdict"]
    for key in sorted(parent[0], key=lambda k: (int(k[1].split("x")[0]), k[0])):
        p, t = [r[key] for r in parent], [r[key] for r in this]
        spread, diff = max(p) - min(p), statistics.median(t) - statistics.median(p)
        lines.append(f"{key[0]:<16}{key[1]:>11}  {' '.join(f'{x:.4f}' for x in p):<34}{' '.join(f'{x:.4f}' for x in t):<34}{spread:>15.4f}"
                     f"{diff:>+13.4f}  {'within the spread' if diff <= spread else 'SLOWER THAN THE SPREAD'}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_bc1_ms.txt"))
    ap.add_argument("--parent-runs", nargs="*", default=[])
    ap.add_argument("--this-runs", nargs="*", default=[])
    ap.add_argument("--sizes", default="1440x960,3840x2160")
    a = ap.parse_args()
    import common
    from direct12pbrrenderer_amd import scene
    from direct12pbrrenderer_amd.api import PbrContext
    from direct12pbrrenderer_amd.pipeline import DeferredFrame, TileSpec
    from direct12pbrrenderer_amd.structs import TEX_BC1_BLOCKS, texture2d_bytes
    from oracle import binding as orc
    from raster_ms import timed

    ctx = PbrContext(0)
    rng = np.random.default_rng(2024)
    sky, env, lut, sh = common.small_ibl(orc)
    rec = common.reference_scene_lights()
    lights = np.concatenate([scene.make_lights(rec["translation"][j], rec["color"][j], rec["radius"][j], rec["intensity"][j])
                             for j in range(len(rec["radius"]))])
    fx = np.load(os.path.join(ROOT, "tests", "golden", "sphere_grid.npz"))
    fxt = np.load(os.path.join(ROOT, "tests", "golden", "textured_models.npz"))
    ms = scene.MeshScene()
    scene.reference_models(fx, ms)
    scene.add_textured_models(ms, fxt)
    v, i, d = ms.arrays()
    maps = ms.maps()
    # the fixture's texture table order, each map as random blocks at the asset's size, level count and stored format
    infos = [tuple(int(x) for x in fxt[f"{n}_{k}_info"][:4]) for n in fxt["name"] for k in fxt["maps"] if f"{n}_{k}_info" in fxt.files]
    bc1 = [ctx.upload_texture(rng.integers(0, 256, texture2d_bytes(w0, h0, m0, fmt | TEX_BC1_BLOCKS), dtype=np.uint8), w0, h0, m0,
                              fmt | TEX_BC1_BLOCKS) for w0, h0, m0, fmt in infos]

    def decode_all():
        return [ctx.bc1_decode(p, w0, h0, m0, fmt) for p, (w0, h0, m0, fmt) in zip(bc1, infos)]
    decoded = decode_all()                                        # (warm-up pass; these chains are the decoded-resident table)
    outs = [t[0] for t in decoded]
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for p, (w0, h0, m0, fmt), o in zip(bc1, infos, outs):         # one pass over the table into the same chains
        ctx.bc1_decode(p, w0, h0, m0, fmt, out=o)
    e1.record()
    torch.cuda.synchronize()
    decode_ms = e0.elapsed_time(e1)
    bytes_bc1 = sum(texture2d_bytes(w0, h0, m0, fmt | TEX_BC1_BLOCKS) for w0, h0, m0, fmt in infos)
    bytes_dec = sum(texture2d_bytes(*inf) for inf in infos)

    lines = [f"pbr_gbuffer_raster with maps, BC1-resident against decoded-resident textures, {torch.cuda.get_device_name(0)}, HIP events, "
             f"{a.iters} calls after 5 warm-up calls",
             "scene: the 33 constant models + barrel, rock, suitcase, tile (fixture meshes; 20 maps of seeded random BC1 blocks at the "
             "assets' sizes, levels and stored formats: 1024^2 x 11 / 2048^2 x 12); the planes of the two rows are equal (checked)",
             f"pbr_bc1_decode, the whole table once ({len(infos)} chains, {bytes_bc1} -> {bytes_dec} bytes): {decode_ms:.4f} ms",
             f"{'row':<18}{'size':>11}{'triangles':>11}{'raster ms':>11}{'texture bytes':>15}{'covered':>9}{'textured px':>13}"]
    for w, h in (tuple(int(x) for x in s.split("x")) for s in a.sizes.split(",")):
        g = scene.make_global(scene.Camera.reference_default(w, h), w, h, sh_pack=sh)

        def dev_half(x):
            return ctx.upload(np.ascontiguousarray(x, dtype=np.float16).view(np.uint16)).view(torch.float16)
        frames = {}
        for row, table in (("decoded-resident", decoded), ("BC1-resident", bc1)):
            fr = DeferredFrame(ctx, TileSpec(0, 0, w, h, w, h, 0), g, lights, dev_half(lut), lut.shape[0], dev_half(env),
                               common.ENV_SIZE, common.ENV_MIPS)
            fr.set_meshes(v, i, d, maps=maps, textures=table)
            fr.rasterize()
            frames[row] = fr
        torch.cuda.synchronize()
        for k in ("A", "B", "C", "depth", "stencil"):
            assert torch.equal(frames["decoded-resident"].gb[k], frames["BC1-resident"].gb[k]), f"{w}x{h}: plane {k} differs"
        times = {row: [] for row in frames}
        for _ in range(3):                                        # the rows alternate: three timed windows each
            for row, fr in frames.items():
                times[row].append(timed(fr.rasterize, a.iters))
        for row, fr in frames.items():
            cov = float((fr.gb["stencil"] > 0).float().mean())
            ao = int(((fr.gb["C"] >> 16) & 255).gt(0).sum())
            nbytes = bytes_dec if row == "decoded-resident" else bytes_bc1
            lines.append(f"{row:<18}{f'{w}x{h}':>11}{fr.mesh['max_triangles']:>11}{statistics.median(times[row]):>11.4f}{nbytes:>15}{cov:>9.3f}{ao:>13}"
                         f"   (windows: {' '.join(f'{t:.4f}' for t in times[row])})")
            print(lines[-1], flush=True)
        frames.clear()
        torch.cuda.empty_cache()
    ctx.close()
    if a.parent_runs and a.this_runs:
        lines += regression_lines(a.parent_runs, a.this_runs)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
