#!/usr/bin/env python3
"""Times pbr_equirect_to_cube with HIP events on the context's stream after warm-up and writes profiles/equirect_ms.txt.

Rows: an 8192 x 4096 panorama -> a 2048^2 cube at samples 1 and 2, and a 4096 x 2048 panorama -> 1024^2 at samples 1, 2 and 4, each
from an fp32 source and from an RGBE source of the same image (seeded noise bytes: uniform mantissas, exponents 120 .. 139; the fp32
source is pbr_rgbe_decode of them, so both rows resample the same texels and write the same bits).  Per row the median of three
windows of --iters calls, the output texels and sub-samples per second, and the bytes a call cannot avoid (the panorama read once +
the cube written once) against the streaming rate measured in the same run (a device-to-device copy of 256 MiB, read + write bytes
over its time).  Then pbr_rgbe_decode of each panorama (what an fp32 source made from a .hdr file costs first), which source format wins
per shape, with and without that decode, and the eight instantiations' register, occupancy and scratch figures as the
compiler reports them.  There is no pass mark on time: nobody has measured this kernel before.
Usage: python tools/equirect_ms.py [--iters N] [--out profiles/equirect_ms.txt]"""
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
HBM_PEAK = 8.0e12
CASES = [(8192, 4096, 2048, (1, 2)), (4096, 2048, 1024, (1, 2, 4))]


def resource_usage():
    """the eight instantiations' figures from -Rpass-analysis=kernel-resource-usage (a compile of the one translation unit, nothing is kept)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return ["kernel resource usage: not measured (no hipcc here)"]
    src = os.path.join(ROOT, "direct12pbrrenderer_amd", "csrc", "equirect.hip")
    with tempfile.TemporaryDirectory() as tmp:
        run = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only",
                              "-Rpass-analysis=kernel-resource-usage", "-S", src, "-o", os.path.join(tmp, "x.s")], capture_output=True, text=True)
        asm = open(os.path.join(tmp, "x.s")).read() if os.path.exists(os.path.join(tmp, "x.s")) else ""
    code = {(int(s), b): int(n) for s, b, n in re.findall(r"^\s*\.type\s+\S*?k_equirect_to_cubeILi(\d)ELb([01])E\S*,@function.*?; codeLenInByte = (\d+)", asm, re.S | re.M)}
    out = []
    for part in run.stderr.split("remark: Function Name: ")[1:]:
        m = re.match(r"\S*k_equirect_to_cubeILi(\d)ELb([01])E", part)
        if not m:
            continue
        got = dict(re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", part))
        out.append(f"k_equirect_to_cube<{m.group(1)}, {'RGBE' if m.group(2) == '1' else 'fp32'}>, gfx950 (-Rpass-analysis=kernel-resource-usage): VGPRs {got.get('VGPRs')}, "
                   f"AGPRs {got.get('AGPRs')}, SGPRs {got.get('TotalSGPRs')}, occupancy {got.get('Occupancy')} waves/SIMD, scratch {got.get('ScratchSize')} bytes/lane, "
                   f"LDS {got.get('LDS Size')} bytes/block, code {code.get((int(m.group(1)), m.group(2)), 'not measured')} bytes")
    return out or ["kernel resource usage: not measured (the compile reported nothing)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "equirect_ms.txt"))
    a = ap.parse_args()
    from direct12pbrrenderer_amd.api import PbrContext
    from raster_ms import timed

    ctx = PbrContext(0)
    rng = np.random.default_rng(2026)

    src = ctx.empty((1 << 28,), torch.uint8)
    src.fill_(3)
    dst = torch.empty_like(src)
    copy_ms = statistics.median([timed(lambda: dst.copy_(src), 50) for _ in range(3)])
    stream = 2.0 * src.numel() / (copy_ms * 1e-3)
    del src, dst
    torch.cuda.empty_cache()

    lines = [f"pbr_equirect_to_cube, {torch.cuda.get_device_name(0)}, HIP events on the context's stream, median of three windows of {a.iters} calls after 5 "
             f"warm-up calls each; the two source formats alternate window by window",
             f"streaming rate measured here: device-to-device copy of 256 MiB, {copy_ms:.4f} ms -> {stream / 1e12:.2f} TB/s read + write "
             f"({100 * stream / HBM_PEAK:.0f} % of the 8 TB/s HBM peak)",
             "moved = panorama bytes (read once) + cube bytes written; of copy = moved / time against the copy's rate",
             f"{'panorama -> cube':<24}{'samples':>8}{'source':>8}{'ms':>10}{'Mtexels/s':>11}{'Msamples/s':>12}{'moved':>12}{'of copy':>9}   windows"]
    verdict, decode = [], []
    for pw, ph, size, sample_counts in CASES:
        rgbe_host = rng.integers(0, 256, size=(ph, pw, 4), dtype=np.uint8)
        rgbe_host[..., 3] = rng.integers(120, 140, size=(ph, pw), dtype=np.uint8)
        rgbe = ctx.upload(rgbe_host)
        del rgbe_host
        fp32 = ctx.empty((ph, pw, 4), torch.float32)
        ctx.rgbe_decode(rgbe, fp32)
        outs = {"fp32": ctx.empty((6 * size * size, 4), torch.float32), "RGBE": ctx.empty((6 * size * size, 4), torch.float32)}
        ctx.sync()
        decode_ms = statistics.median([timed(lambda: ctx.rgbe_decode(rgbe, fp32), a.iters) for _ in range(3)])
        decode.append(f"pbr_rgbe_decode of the {pw}x{ph} panorama, what an fp32 source made from a .hdr costs in front of the resampling: {decode_ms:.4f} ms "
                      f"({100 * 20 * pw * ph / (decode_ms * 1e-3) / stream:.0f} % of the copy's rate on its 4 + 16 bytes a texel)")
        for samples in sample_counts:
            calls = {"fp32": lambda: ctx.equirect_to_cube(fp32, pw, ph, size, samples, out=outs["fp32"]),
                     "RGBE": lambda: ctx.equirect_to_cube(rgbe, pw, ph, size, samples, rgbe=True, out=outs["RGBE"])}
            times = {k: [] for k in calls}
            for _ in range(3):
                for k, fn in calls.items():
                    times[k].append(timed(fn, a.iters))
            ctx.sync()
            same = bool(torch.equal(outs["fp32"].view(torch.int32), outs["RGBE"].view(torch.int32)))
            med = {k: statistics.median(v) for k, v in times.items()}
            for k in calls:
                moved = pw * ph * (16 if k == "fp32" else 4) + 96 * size * size
                texels = 6 * size * size
                lines.append(f"{f'{pw}x{ph} -> {size}^2':<24}{samples:>8}{k:>8}{med[k]:>10.4f}{texels / (med[k] * 1e-3) / 1e6:>11.1f}"
                             f"{texels * samples * samples / (med[k] * 1e-3) / 1e6:>12.1f}{moved:>12}{100 * moved / (med[k] * 1e-3) / stream:>8.2f}%   "
                             f"{' '.join(f'{t:.4f}' for t in times[k])}")
                print(lines[-1], flush=True)
            verdict.append(f"{pw}x{ph} -> {size}^2, samples {samples}: RGBE time / fp32 time {med['RGBE'] / med['fp32']:.3f}, "
                           f"/ (decode + fp32) time {med['RGBE'] / (decode_ms + med['fp32']):.3f}; outputs bit-identical: {same}")
        del rgbe, fp32, outs
        torch.cuda.empty_cache()
    ctx.close()
    lines += [""] + decode + verdict + [""] + resource_usage()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
