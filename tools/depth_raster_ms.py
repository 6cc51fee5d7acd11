#!/usr/bin/env python3
"""Times pbr_depth_raster against pbr_gbuffer_raster (the shadow pass's two paths) in one process and writes profiles/depth_raster_ms.txt.

Scene: the reference mesh scene (tests/golden/sphere_grid.npz: 33 constant-material models), sun (1, 1, 1).  Cases: the shadow map under
the light camera pbr_sun_fit fits around the draws' world boxes, at 1024^2 and 2048^2, and the camera's own 1440 x 960 view as a depth
pre-pass.  Per case the two calls alternate: every shape is warmed, then --reps repetitions of each, every repetition --iters calls
between two device events and a synchronise; the row is the median with its range (min .. max).  Both depth planes are compared bit for
bit before anything is timed.  Counted from the shapes, not measured: the bytes each call writes to its target (17 B against 4 B per
texel) and the scratch sizes.  Last, DeferredFrame.shadow_pass() itself at 2048^2 in both modes, the row profiles/sun_light_ms.txt calls
"shadow raster (fit + 6 launches)": the light-camera fit and the Python call path on the host, then the same six launches; and the host
clock around one call without any device wait, which shows how much of that row is the host's.  There is no pass mark on time.

--trace: no timing and no file; both chains run --reps times at 2048^2, for a run under the profiler
(rocprofv3 --kernel-trace --stats -- python tools/depth_raster_ms.py --trace), which gives the time per launch.
Usage: python tools/depth_raster_ms.py [--reps N] [--iters N] [--out profiles/depth_raster_ms.txt] [--trace]"""
import argparse
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import common  # noqa: E402
from direct12pbrrenderer_amd import scene, synth  # noqa: E402
from direct12pbrrenderer_amd.api import PbrContext, sun_fit  # noqa: E402
from direct12pbrrenderer_amd.pipeline import DeferredFrame, TileSpec  # noqa: E402
from oracle import binding as orc  # noqa: E402
from direct12pbrrenderer_amd.structs import Tile  # noqa: E402
from raster_ms import timed  # noqa: E402

MAPS = [1024, 2048]
CAMERA = (1440, 960)
NEW_KERNELS = ("k_rs_depth", "k_rs_fill_depth", "RsSetupDepth")


def resource_usage():
    """the depth chain's own kernels from -Rpass-analysis=kernel-resource-usage (a compile of the one translation unit, nothing is kept)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return ["kernel resource usage: not measured (no hipcc here)"]
    src = os.path.join(ROOT, "direct12pbrrenderer_amd", "csrc", "gbuffer_raster.hip")
    with tempfile.TemporaryDirectory() as tmp:
        run = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                              "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", src, "-o", os.path.join(tmp, "x.s")],
                             capture_output=True, text=True)
    out = []
    for part in run.stderr.split("remark: Function Name: ")[1:]:
        name = part.split()[0]
        hit = next((k for k in NEW_KERNELS if k in name), None)
        if hit is None:
            continue
        got = dict(re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", part))
        shown = "k_rs_setup<RsSetupDepth>" if hit == "RsSetupDepth" else hit
        out.append(f"{shown}, gfx950 (-Rpass-analysis=kernel-resource-usage): VGPRs {got.get('VGPRs')} (spilled {got.get('VGPRs Spill')}), "
                   f"SGPRs {got.get('TotalSGPRs')} (spilled {got.get('SGPRs Spill')}), LDS {got.get('LDS Size')} bytes/block, "
                   f"scratch {got.get('ScratchSize')} bytes/lane, occupancy {got.get('Occupancy')} waves/SIMD")
    return out or ["kernel resource usage: not measured (the compile reported nothing)"]


def spread(ms):
    return f"{statistics.median(ms):.4f} ({min(ms):.4f} .. {max(ms):.4f})"


def shadow_pass_rows(ctx, v, i, d, a):
    """DeferredFrame.shadow_pass() at 2048^2, depth_only off and on: device events as above, and the host's own time per call"""
    sky, env, lut, sh = common.small_ibl(orc)

    def dev_half(x):
        return ctx.upload(np.ascontiguousarray(x, dtype=np.float16).view(np.uint16)).view(torch.float16)
    w, h = CAMERA
    g = scene.make_global(scene.Camera.reference_default(w, h), w, h, sh_pack=sh)
    frames = {}
    for only in (False, True):
        fr = DeferredFrame(ctx, TileSpec(0, 0, w, h, w, h, 0), g, synth.reference_scene_light(), dev_half(lut), lut.shape[0], dev_half(env),
                           common.ENV_SIZE, common.ENV_MIPS)
        fr.set_meshes(v, i, d)
        fr.set_sun((1.0, 1.0, 1.0), 100.0, map_size=2048, pcf=3, depth_only=only)
        timed(fr.shadow_pass, a.iters)
        frames[only] = fr
    res, host = {False: [], True: []}, {False: [], True: []}
    for _ in range(a.reps):
        for only, fr in frames.items():
            res[only].append(timed(fr.shadow_pass, a.iters, warm=1))
            ctx.sync()
            t0 = time.perf_counter()
            for _k in range(a.iters):
                fr.shadow_pass()
            host[only].append((time.perf_counter() - t0) * 1e3 / a.iters)      # enqueue only: no device wait inside
            ctx.sync()
    same = bool(torch.equal(frames[False].shadow_map()[0].view(torch.int32), frames[True].shadow_map()[0].view(torch.int32)))
    out = [f"DeferredFrame.shadow_pass() at 2048^2 (light-camera fit on the host + the six launches), same bits: {'yes' if same else 'NO'}"]
    for only, name in ((False, "depth_only=False"), (True, "depth_only=True")):
        out.append(f"  {name:<18}{spread(res[only]):>30} ms between device events; the host alone, per call: {spread(host[only])} ms")
    return out + [""]


class Case:
    """one target under one camera: both calls on buffers of their own"""

    def __init__(self, ctx, name, g, w, h, dev, n_tris):
        self.ctx, self.name, self.g, self.w, self.h, self.dev, self.n = ctx, name, g, w, h, dev, n_tris
        self.tile = Tile(0, 0, w, h, w, h)
        self.planes = [ctx.zeros((h, w), torch.int32) for _ in range(3)] + [ctx.zeros((h, w), torch.float32), ctx.zeros((h, w), torch.uint8)]
        self.scratch = ctx.alloc_raster_scratch(w, h, n_tris)
        self.depth = ctx.zeros((h, w), torch.float32)
        self.depth_scratch = ctx.alloc_depth_raster_scratch(w, h, n_tris)

    def gbuffer(self):
        self.ctx.gbuffer_raster(self.g, self.tile, *self.dev, self.n, *self.planes, self.w, self.scratch)

    def depth_only(self):
        self.ctx.depth_raster(self.g, self.tile, *self.dev, self.n, self.depth, self.w, self.depth_scratch)

    def same_bits(self):
        self.gbuffer()
        self.depth_only()
        self.ctx.sync()
        return bool(torch.equal(self.planes[3].view(torch.int32), self.depth.view(torch.int32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_raster_ms.txt"))
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    assert a.reps >= 30 or a.trace, "at least 30 timed repetitions per path"
    assert torch.cuda.is_available(), "depth_raster_ms.py measures on the GPU; there is none here"
    ctx = PbrContext(0)
    fx = np.load(os.path.join(ROOT, "tests", "golden", "sphere_grid.npz"))
    (v, i, d), _ = scene.reference_models(fx)
    n_tris = int((d["index_count"] // 3).sum())
    dev = (ctx.upload(v), len(v), ctx.upload(i), len(i), ctx.upload(d), len(d))
    mn, mx = scene.world_box(d, scene.draw_bounds(v, i, d))
    direction = (np.ones(3) / np.sqrt(3.0)).astype(np.float32)

    def light_case(n):
        return Case(ctx, f"shadow map {n}^2", sun_fit(direction, mn, mx, n, n)[0], n, n, dev, n_tris)

    if a.trace:
        case = light_case(2048)
        assert case.same_bits()
        for _ in range(a.reps):
            case.gbuffer()
            case.depth_only()
        ctx.sync()
        ctx.close()
        print(f"trace run: {a.reps + 1} calls of each chain at 2048^2")
        return

    lines = [f"pbr_depth_raster against pbr_gbuffer_raster, {torch.cuda.get_device_name(0)}, device events ending in a synchronise; median (min .. max) "
             f"of {a.reps} repetitions of {a.iters} calls per path, the two paths alternating, after warm-up of every shape",
             f"scene: the reference mesh scene, {len(d)} draws, {n_tris} triangles; sun (1, 1, 1); both calls in this one process, recommended scratch",
             "target bytes and scratch sizes are counted from the shapes; the depth planes of the two calls were compared bit for bit first", ""]
    w, h = CAMERA
    cases = [light_case(n) for n in MAPS] + [Case(ctx, f"camera {w}x{h} (depth pre-pass)", scene.make_global(scene.Camera.reference_default(w, h), w, h),
                                                  w, h, dev, n_tris)]
    for case in cases:
        assert case.same_bits(), f"{case.name}: the depth planes differ"
        covered = float((case.depth < 1.0).float().mean())
        res = {"gbuffer": [], "depth": []}
        for fn in (case.gbuffer, case.depth_only):
            timed(fn, a.iters)
        for _ in range(a.reps):
            res["gbuffer"].append(timed(case.gbuffer, a.iters, warm=1))
            res["depth"].append(timed(case.depth_only, a.iters, warm=1))
        texels = case.w * case.h
        mg, md = statistics.median(res["gbuffer"]), statistics.median(res["depth"])
        lines += [f"{case.name}: {100.0 * covered:.1f} % of the texels covered, same bits: yes",
                  f"  pbr_gbuffer_raster  {spread(res['gbuffer']):>30} ms   target {17 * texels / 1e6:7.1f} MB written (17 B / texel), scratch "
                  f"{case.scratch.numel() / 1e6:6.2f} MB",
                  f"  pbr_depth_raster    {spread(res['depth']):>30} ms   target {4 * texels / 1e6:7.1f} MB written ( 4 B / texel), scratch "
                  f"{case.depth_scratch.numel() / 1e6:6.2f} MB",
                  f"  depth / gbuffer = {md / mg:.3f} of the time; scratch smaller by {(case.scratch.numel() - case.depth_scratch.numel()) / 1e6:.2f} MB", ""]
    del cases
    torch.cuda.empty_cache()
    lines += shadow_pass_rows(ctx, v, i, d, a)
    lines += resource_usage()
    ctx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
