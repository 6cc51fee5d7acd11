#!/usr/bin/env python3
"""Times pbr_sun_light with device events after warm-up and writes profiles/sun_light_ms.txt.

Sizes 1440 x 960 and 3840 x 2160 on the reference mesh scene (tests/golden/sphere_grid.npz through DeferredFrame.set_meshes: 33
constant-material models, reference camera, the reference's own directional light: direction (1, 1, 1), 100 nits), a 2048^2 shadow map
fitted around the draws' world boxes.  Per size: the pass with pcf 1, pcf 3 and without a map, the shadow raster itself
(pbr_gbuffer_raster under the light's camera), and as the scale pbr_tonemap and the one-light shade of the same frame, all in
alternating windows of the same run.  Per row: the median of --windows windows of --iters calls with their spread (min .. max), and
for the sun pass the bytes a call cannot avoid (33 per geometry pixel: 17 of G-buffer read, 8 of HDR read and 8 written; pixels
without geometry read their stencil byte only) over the time as a share of the device-to-device copy rate measured in the same run.
There is no pass mark on time.
Usage: python tools/sun_light_ms.py [--iters N] [--windows N] [--out profiles/sun_light_ms.txt]"""
import argparse
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import common  # noqa: E402
from direct12pbrrenderer_amd import scene, synth  # noqa: E402
from direct12pbrrenderer_amd.api import PbrContext, make_sun  # noqa: E402
from direct12pbrrenderer_amd.pipeline import DeferredFrame, TileSpec  # noqa: E402
from oracle import binding as orc  # noqa: E402
from raster_ms import timed  # noqa: E402

SIZES = [(1440, 960), (3840, 2160)]
MAP = 2048


def resource_usage():
    """k_sun_light's figures from -Rpass-analysis=kernel-resource-usage (a compile of the one translation unit, nothing is kept)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return ["kernel resource usage: not measured (no hipcc here)"]
    src = os.path.join(ROOT, "direct12pbrrenderer_amd", "csrc", "sun.hip")
    with tempfile.TemporaryDirectory() as tmp:
        run = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                              "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", src, "-o", os.path.join(tmp, "x.s")],
                             capture_output=True, text=True)
    out = []
    for part in run.stderr.split("remark: Function Name: ")[1:]:
        m = re.match(r"\S*k_sun_lightILb([01])E", part)
        if not m:
            continue
        got = dict(re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", part))
        out.append(f"k_sun_light<{'probe' if m.group(1) == '1' else 'hdr'}>, gfx950 (-Rpass-analysis=kernel-resource-usage): VGPRs {got.get('VGPRs')}, "
                   f"SGPRs {got.get('TotalSGPRs')}, LDS {got.get('LDS Size')} bytes/block, scratch {got.get('ScratchSize')} bytes/lane, "
                   f"occupancy {got.get('Occupancy')} waves/SIMD")
    return out or ["kernel resource usage: not measured (the compile reported nothing)"]


def windows(fns, iters, n):
    out = [[] for _ in fns]
    for _ in range(n):
        for k, fn in enumerate(fns):
            if getattr(fn, "before", None):
                fn.before()
            out[k].append(timed(fn, iters))
    return out


def spread(ms):
    return f"{statistics.median(ms):.4f} ({min(ms):.4f} .. {max(ms):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sun_light_ms.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sun_light_ms.py measures on the GPU; there is none here"
    ctx = PbrContext(0)

    big = ctx.empty((1 << 28,), torch.uint8)
    big.fill_(3)
    other = torch.empty_like(big)
    copy_ms = statistics.median([timed(lambda: other.copy_(big), 50) for _ in range(3)])
    copy_rate = 2.0 * big.numel() / (copy_ms * 1e-3)
    del big, other
    torch.cuda.empty_cache()

    sky, env, lut, sh = common.small_ibl(orc)

    def dev_half(x):
        return ctx.upload(np.ascontiguousarray(x, dtype=np.float16).view(np.uint16)).view(torch.float16)
    fx = np.load(os.path.join(ROOT, "tests", "golden", "sphere_grid.npz"))
    (v, i, d), _ = scene.reference_models(fx)
    lines = [f"pbr_sun_light, {torch.cuda.get_device_name(0)}, device events, median (min .. max) of {a.windows} windows of {a.iters} calls after 5 "
             f"warm-up calls each; the windows of a size's rows alternate",
             f"scene: the reference mesh scene, {len(d)} draws, {int((d['index_count'] // 3).sum())} triangles; sun (1, 1, 1), shadow map {MAP}^2 "
             f"(its raster writes a scratch G-buffer of 17 B per texel: {17 * MAP * MAP / 1e6:.0f} MB)",
             f"copy rate measured here: device-to-device copy of 256 MiB, {copy_ms:.4f} ms -> {copy_rate / 1e12:.2f} TB/s read + write",
             "moved = 33 bytes per geometry pixel + 1 per other pixel; of copy = moved / time against the copy's rate", ""]
    for w, h in SIZES:
        cam = scene.Camera.reference_default(w, h)
        g = scene.make_global(cam, w, h, sh_pack=sh)
        fr = DeferredFrame(ctx, TileSpec(0, 0, w, h, w, h, 0), g, synth.reference_scene_light(), dev_half(lut), lut.shape[0], dev_half(env),
                           common.ENV_SIZE, common.ENV_MIPS)
        fr.set_meshes(v, i, d)
        fr.set_prev_luminance(0.18)
        fr.set_sun((1.0, 1.0, 1.0), 100.0, map_size=MAP, pcf=3)
        fr.render()
        ctx.sync()
        geometry = int((fr.gb["stencil"] > 0).sum())
        moved = 33.0 * geometry + (w * h - geometry)
        depth, mw, mh, mp, lvp = fr.shadow_map()
        bias = DeferredFrame.SUN_BIAS
        sun3 = make_sun((1.0, 1.0, 1.0), 100.0, lvp, bias, 3)
        sun1 = make_sun((1.0, 1.0, 1.0), 100.0, lvp, bias, 1)
        shaded = fr.hdr.clone()      # the target as the pass finds it in a frame; restored before every window (the pass accumulates)
        hdr = shaded.clone()
        probe = ctx.zeros((h, w, 4), torch.float32)
        ctx.sun_light(g, fr.tile, fr.gb, w, sun3, None, w, depth, mw, mh, mp, contrib_f32=probe)
        ctx.sync()
        lit = probe[..., 3] > 0
        rgb = probe[..., :3].sum(dim=-1)
        shadowed = float(((rgb == 0) & lit).sum()) / max(geometry, 1)

        def sun(s, m):
            fn = sun_call(s, m)
            fn.before = lambda: hdr.copy_(shaded)
            return fn

        def sun_call(s, m):
            return lambda: ctx.sun_light(g, fr.tile, fr.gb, w, s, hdr, w, m, mw if m is not None else 0, mh if m is not None else 0, mp if m is not None else 0)
        names = ["pbr_sun_light pcf 3", "pbr_sun_light pcf 1", "pbr_sun_light no map", "shadow raster (fit + 6 launches)", "pbr_tonemap", "shade, 1 light"]
        res = windows([sun(sun3, depth), sun(sun1, depth), sun(sun3, None), fr.shadow_pass, fr.tonemap, fr.shade], a.iters, a.windows)
        lines.append(f"{w}x{h}: {geometry} geometry pixels ({100.0 * geometry / (w * h):.1f} %), {100.0 * float(lit.sum()) / max(geometry, 1):.1f} % of them "
                     f"face the sun, {100.0 * shadowed:.1f} % fully shadowed")
        for name, ms in zip(names, res):
            med = statistics.median(ms)
            share = f"{moved / (med * 1e-3) / copy_rate:>9.3f} of copy" if name.startswith("pbr_sun") else ""
            lines.append(f"  {name:<34}{spread(ms):>30} ms{share}")
        lines.append("")
        del fr, hdr, probe
        torch.cuda.empty_cache()
    lines += resource_usage()
    ctx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
