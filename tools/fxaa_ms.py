#!/usr/bin/env python3
"""Times pbr_fxaa / pbr_fxaa_batch with device events after warm-up and writes profiles/fxaa_ms.txt.

Sizes 1440 x 960 and 3840 x 2160, three inputs each: the tone-mapped target of a rendered frame of the reference mesh scene
(tests/golden/sphere_grid.npz through DeferredFrame.set_meshes, reference camera, main.json's 8 lights, the small IBL: the figure that
matters), a constant frame (no edge pixel: the streaming floor) and noise (every pixel an edge whose walks end at once: the ceiling).
Per row: the median of --windows windows of --iters calls with their spread (min .. max), the share of edge pixels, the bytes a call
cannot avoid (8 w h: every pixel read once and written once) over the time as a fraction of the device-to-device copy rate measured in
the same run, and pbr_tonemap of the same frame, its windows alternating with the filter's: the yardstick a user holds the pass
against.  Then, at 1440 x 960 on the rendered frame, one batch of 1 and one batch of 8 against 8 sequential calls.  The filtered
rendered frame is compared with the restatement (tests/fxaa_ref.py) before anything is timed.  There is no pass mark on time.
Usage: python tools/fxaa_ms.py [--iters N] [--windows N] [--out profiles/fxaa_ms.txt]"""
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
import fxaa_ref  # noqa: E402
from direct12pbrrenderer_amd import scene  # noqa: E402
from direct12pbrrenderer_amd.api import PbrContext  # noqa: E402
from direct12pbrrenderer_amd.pipeline import DeferredFrame, TileSpec  # noqa: E402
from oracle import binding as orc  # noqa: E402
from raster_ms import timed  # noqa: E402

SIZES = [(1440, 960), (3840, 2160)]


def resource_usage():
    """k_fxaa's figures from -Rpass-analysis=kernel-resource-usage (a compile of the one translation unit, nothing is kept)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return ["kernel resource usage: not measured (no hipcc here)"]
    src = os.path.join(ROOT, "direct12pbrrenderer_amd", "csrc", "fxaa.hip")
    with tempfile.TemporaryDirectory() as tmp:
        run = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only",
                              "-Rpass-analysis=kernel-resource-usage", "-S", src, "-o", os.path.join(tmp, "x.s")], capture_output=True, text=True)
    out = []
    for part in run.stderr.split("remark: Function Name: ")[1:]:
        m = re.match(r"\S*k_fxaaILb([01])E", part)
        if not m:
            continue
        got = dict(re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", part))
        out.append(f"k_fxaa<{'batch' if m.group(1) == '1' else 'single'}>, gfx950 (-Rpass-analysis=kernel-resource-usage): VGPRs {got.get('VGPRs')}, "
                   f"SGPRs {got.get('TotalSGPRs')}, LDS {got.get('LDS Size')} bytes/block, scratch {got.get('ScratchSize')} bytes/lane, "
                   f"occupancy {got.get('Occupancy')} waves/SIMD")
    return out or ["kernel resource usage: not measured (the compile reported nothing)"]


def edge_share(img):
    """the share of pixels that pass the rule's contrast test, on the device (int64 torch arithmetic, clamped reads)"""
    p = img.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    lum = 77 * (p & 255) + 150 * ((p >> 8) & 255) + 29 * ((p >> 16) & 255)
    pad = torch.nn.functional.pad(lum[None, None].to(torch.float64), (1, 1, 1, 1), mode="replicate")[0, 0].to(torch.int64)
    five = torch.stack([pad[1:-1, 1:-1], pad[:-2, 1:-1], pad[2:, 1:-1], pad[1:-1, :-2], pad[1:-1, 2:]])
    hi, lo = five.max(dim=0).values, five.min(dim=0).values
    return float((hi - lo >= torch.clamp(hi >> 3, min=4080)).double().mean())


def windows(fns, iters, n):
    """n windows of every function in turn (A B C A B C ...): -> one list of ms per call per function"""
    out = [[] for _ in fns]
    for _ in range(n):
        for k, fn in enumerate(fns):
            out[k].append(timed(fn, iters))
    return out


def spread(ms):
    return f"{statistics.median(ms):.4f} ({min(ms):.4f} .. {max(ms):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fxaa_ms.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fxaa_ms.py measures on the GPU; there is none here"
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
    rec = common.reference_scene_lights()
    lights = np.concatenate([scene.make_lights(rec["translation"][j], rec["color"][j], rec["radius"][j], rec["intensity"][j])
                             for j in range(len(rec["radius"]))])

    lines = [f"pbr_fxaa, {torch.cuda.get_device_name(0)}, device events, median (min .. max) of {a.windows} windows of {a.iters} calls after 5 warm-up calls "
             f"each; within a block of rows the windows of the filter and of pbr_tonemap alternate",
             f"copy rate measured here: device-to-device copy of 256 MiB, {copy_ms:.4f} ms -> {copy_rate / 1e12:.2f} TB/s read + write",
             "moved = 8 w h bytes (every pixel read once, written once); of copy = moved / time against the copy's rate",
             f"{'size':<12}{'input':<10}{'edge pixels':>12}{'pbr_fxaa ms':>30}{'of copy':>9}{'pbr_tonemap ms':>30}{'fxaa / tonemap':>16}"]
    rendered = {}
    for w, h in SIZES:
        cam = scene.Camera.reference_default(w, h)
        g = scene.make_global(cam, w, h, sh_pack=sh)
        fr = DeferredFrame(ctx, TileSpec(0, 0, w, h, w, h, 0), g, lights, dev_half(lut), lut.shape[0], dev_half(env), common.ENV_SIZE, common.ENV_MIPS)
        fr.set_meshes(v, i, d)
        fr.set_prev_luminance(0.18)
        fr.render(antialias=True)
        ctx.sync()
        if (w, h) == SIZES[0]:      # the restatement takes a while at 4K; the GPU tests hold the kernel to it at every path
            assert np.array_equal(fr.ldr_aa_numpy(), fxaa_ref.fxaa(fr.ldr_numpy())), "the filtered frame differs from the restatement"
        rendered[(w, h)] = fr.ldr.clone()
        const = torch.full_like(fr.ldr, 0x40302010)
        noise = torch.randint(-2 ** 31, 2 ** 31 - 1, (h, w), dtype=torch.int64, device=fr.ldr.device, generator=torch.Generator(fr.ldr.device).manual_seed(7)).to(torch.int32)
        out = torch.empty_like(fr.ldr)
        for name, src in (("rendered", rendered[(w, h)]), ("constant", const), ("noise", noise)):
            ms_f, ms_t = windows([lambda: ctx.fxaa(src, w, h, w, out, w), fr.tonemap], a.iters, a.windows)
            med = statistics.median(ms_f)
            lines.append(f"{f'{w}x{h}':<12}{name:<10}{100 * edge_share(src):>11.2f}%{spread(ms_f):>30}{8.0 * w * h / (med * 1e-3) / copy_rate:>9.3f}"
                         f"{spread(ms_t):>30}{med / statistics.median(ms_t):>16.2f}")
        del fr, const, noise, out
        torch.cuda.empty_cache()

    w, h = SIZES[0]
    srcs = [rendered[(w, h)].clone() for _ in range(8)]
    dsts = [torch.empty_like(s) for s in srcs]
    table = [(s, w, dd, w) for s, dd in zip(srcs, dsts)]

    def sequential():
        for s, dd in zip(srcs, dsts):
            ctx.fxaa(s, w, h, w, dd, w)
    ms_1, ms_8, ms_seq = windows([lambda: ctx.fxaa_batch(table[:1], w, h), lambda: ctx.fxaa_batch(table, w, h), sequential], a.iters, a.windows)
    lines += ["", f"batches at {w}x{h}, rendered frame, the three alternating window by window:",
              f"  pbr_fxaa_batch of 1:      {spread(ms_1)} ms",
              f"  pbr_fxaa_batch of 8:      {spread(ms_8)} ms = {statistics.median(ms_8) / 8:.4f} ms per image",
              f"  8 sequential pbr_fxaa:    {spread(ms_seq)} ms = {statistics.median(ms_seq) / 8:.4f} ms per image; "
              f"batch / sequential = {statistics.median(ms_8) / statistics.median(ms_seq):.3f}", ""]
    lines += resource_usage()
    ctx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
