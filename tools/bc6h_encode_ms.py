#!/usr/bin/env python3
"""Times pbr_bc6h_encode_cube and pbr_bc6h_encode_cube_ex with PBR_BC6H_ENCODE_TWO_REGION, alternated window by window on the same
cube, with HIP events on the context's stream after warm-up, and writes profiles/bc6h_encode_ms.txt.

Rows: cubes of 512^2, 1024^2 and 2048^2 with their full chains (box mips from pbr_cube_gen_mips), two kinds of input each, timed
separately because refinement and mode acceptance diverge between them:
  smooth   the analytic sky of tests/golden/make_sky_bc6h.py (gradient + a sun lobe); above 512^2 the 512^2 faces are tiled, so every
           block is still a smooth one (a tile's edge is a block's edge);
  noise    seeded heavy-tailed noise, random ** 4 * 200: every block spans decades, refinement runs twice, few blocks fit a delta.
The two-region row carries its time over the one-region row's (the ratio) and both carry their mode histogram.
Per row the median of three windows of --iters calls, blocks/s, and the bytes moved (fp32 texels read + blocks written) against the
streaming rate measured in the same run (a device-to-device copy of 256 MiB, read + write bytes over its time).  Beside them, in the
same run: pbr_bc1_encode at an equal block count (an S x 6 S RGBA8 chain for a cube of edge S) and pbr_bc6h_decode_cube of the
encoder's result.  Then the encoder's squared error against the test-side yardstick bc6h_ref.encode_mode3 on the 32^2 fixture and
the two-region rule's error over the one-region rule's, level by level (numpy, no GPU), and both kernels' register, occupancy,
code-size and scratch figures as the compiler reports them.  There is no pass mark on time.
Usage: python tools/bc6h_encode_ms.py [--iters N] [--sizes 512 1024 2048] [--out profiles/bc6h_encode_ms.txt]"""
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")]
HBM_PEAK = 8.0e12
SMOOTH_EDGE = 512


def resource_usage():
    """both kernels' figures from -Rpass-analysis=kernel-resource-usage and the code length the compiler writes beside its assembly (a
    compile of the one translation unit, nothing is kept)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return "kernel resource usage: not measured (no hipcc here)"
    src = os.path.join(ROOT, "direct12pbrrenderer_amd", "csrc", "bc6h_encode.hip")
    with tempfile.TemporaryDirectory() as tmp:
        run = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only",
                              "-Rpass-analysis=kernel-resource-usage", "-S", src, "-o", os.path.join(tmp, "x.s")], capture_output=True, text=True)
        asm = open(os.path.join(tmp, "x.s")).read() if os.path.exists(os.path.join(tmp, "x.s")) else ""
    code = dict(re.findall(r"^\s*\.type\s+\S*?(k_bc6h_encode_cube2?)E\S*,@function.*?; codeLenInByte = (\d+)", asm, re.S | re.M))
    out = []
    for part in run.stderr.split("remark: Function Name: ")[1:]:
        name = "k_bc6h_encode_cube2" if "k_bc6h_encode_cube2E" in part.split()[0] else "k_bc6h_encode_cube"
        got = dict(re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", part))
        out.append(f"{name}, gfx950 (-Rpass-analysis=kernel-resource-usage): VGPRs {got.get('VGPRs')}, AGPRs {got.get('AGPRs')}, SGPRs {got.get('TotalSGPRs')}, "
                   f"occupancy {got.get('Occupancy')} waves/SIMD, scratch {got.get('ScratchSize')} bytes/lane, VGPR spills {got.get('VGPRs Spill')}, "
                   f"SGPR spills (to VGPR lanes) {got.get('SGPRs Spill')}, LDS {got.get('LDS Size')} bytes/block, code {code.get(name, 'not measured')} bytes")
    return "\n".join(out) if out else "kernel resource usage: not measured (the compile reported nothing)"


def quality_lines():
    import bc6h_encode2_ref as enc2
    import bc6h_encode_ref as enc
    import bc6h_ref
    smooth = dict(np.load(os.path.join(ROOT, "tests", "golden", "sky_bc6h.npz"), allow_pickle=False))["smooth_level0"]
    ratios, ratios2, won = [], [], []
    for img in enc.box_mips(smooth, 6):
        ours = theirs = two = 0
        for f in range(6):
            h, inside = enc.level_texels(img[f])
            err = lambda b: int(np.where(inside[..., None], (bc6h_ref.decode_blocks(b) - h) ** 2, 0).sum())   # noqa: E731
            ours, theirs = ours + err(enc.encode_level(img[f])[0]), theirs + err(bc6h_ref.encode_mode3(img[f]))
        blocks, _, mode, _ = enc2.encode_level6(img)
        for f in range(6):
            h, inside = enc.level_texels(img[f])
            two += int(np.where(inside[..., None], (bc6h_ref.decode_blocks(blocks[f]) - h) ** 2, 0).sum())
        ratios.append(ours / theirs)
        ratios2.append(two / ours if ours else 0.0)
        won.append(f"{int(np.isin(mode, enc2.TWO_REGION).sum())} of {mode.size}")
    return ["squared error in half-code space against the yardstick bc6h_ref.encode_mode3, the 32^2 fixture sky, levels 32 .. 1 (numpy restatement, "
            "which the kernel equals bit for bit): " + ", ".join(f"{r:.3f}" for r in ratios),
            "two-region rule's error / one-region rule's error, the same levels (numpy restatements, decoded by bc6h_ref.decode_blocks): "
            + ", ".join(f"{r:.3f}" for r in ratios2) + "; blocks that took a two-region mode: " + ", ".join(won)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--sizes", type=int, nargs="*", default=[512, 1024, 2048])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bc6h_encode_ms.txt"))
    a = ap.parse_args()
    import bc6h_ref
    from direct12pbrrenderer_amd.api import PbrContext
    from direct12pbrrenderer_amd.structs import bc6h_chain_bytes, cube_texels, texture2d_bytes
    from make_sky_bc6h import analytic_sky
    from raster_ms import timed

    ctx = PbrContext(0)
    rng = np.random.default_rng(2026)

    def windows(fn):
        return [timed(fn, a.iters) for _ in range(3)]

    src = ctx.empty((1 << 28,), torch.uint8)
    src.fill_(3)
    dst = torch.empty_like(src)
    copy_ms = statistics.median([timed(lambda: dst.copy_(src), 50) for _ in range(3)])
    stream = 2.0 * src.numel() / (copy_ms * 1e-3)
    del src, dst
    torch.cuda.empty_cache()

    lines = [f"pbr_bc6h_encode_cube and pbr_bc6h_encode_cube_ex(PBR_BC6H_ENCODE_TWO_REGION), {torch.cuda.get_device_name(0)}, HIP events on the "
             f"context's stream, median of three windows of {a.iters} calls after 5 warm-up calls each; the two encoders alternate window by window",
             f"streaming rate measured here: device-to-device copy of 256 MiB, {copy_ms:.4f} ms -> {stream / 1e12:.2f} TB/s read + write "
             f"({100 * stream / HBM_PEAK:.0f} % of the 8 TB/s HBM peak)",
             "moved = input bytes read + output bytes written; of copy = moved / time against the copy's rate",
             f"{'call':<28}{'cube / chain':>18}{'input':>8}{'ms':>10}{'blocks':>10}{'Mblocks/s':>11}{'moved':>12}{'of copy':>9}   windows"]

    def row(call, what, kind, ms, blocks, moved):
        med = statistics.median(ms)
        lines.append(f"{call:<28}{what:>18}{kind:>8}{med:>10.4f}{blocks:>10}{blocks / (med * 1e-3) / 1e6:>11.1f}{moved:>12}"
                     f"{100 * moved / (med * 1e-3) / stream:>8.2f}%   {' '.join(f'{t:.4f}' for t in ms)}")
        print(lines[-1], flush=True)

    sky = analytic_sky(min(max(a.sizes), SMOOTH_EDGE))
    for size in a.sizes:
        mips = size.bit_length()
        n = bc6h_chain_bytes(size, mips)
        texels = cube_texels(size, mips)
        cube = ctx.empty((texels, 4), torch.float32)
        faces, faces2 = [ctx.empty((n,), torch.uint8) for _ in range(6)], [ctx.empty((n,), torch.uint8) for _ in range(6)]
        back = ctx.empty((texels, 4), torch.float32)
        for kind in ("smooth", "noise"):
            lv = np.ones((6, size, size, 4), np.float32)
            if kind == "smooth":
                e = min(size, sky.shape[1])
                lv[..., :3] = np.tile(analytic_sky(e) if e != sky.shape[1] else sky, (1, size // e, size // e, 1))
            else:
                lv[..., :3] = rng.random((6, size, size, 3), dtype=np.float32) ** 4 * 200
            cube[:6 * size * size].copy_(torch.from_numpy(lv.reshape(-1, 4)))
            del lv
            ctx.cube_gen_mips(cube, size, mips)
            ctx.sync()
            calls = {"pbr_bc6h_encode_cube": lambda: ctx.bc6h_encode_cube(cube, size, mips, out=faces),
                     "..._ex TWO_REGION": lambda: ctx.bc6h_encode_cube(cube, size, mips, out=faces2, two_region=True)}
            times = {call: [] for call in calls}
            for _ in range(3):                                    # the two alternate: three timed windows each
                for call, fn in calls.items():
                    times[call].append(timed(fn, a.iters))
            ctx.sync()
            for call, out in (("pbr_bc6h_encode_cube", faces), ("..._ex TWO_REGION", faces2)):
                row(call, f"{size}^2 x {mips}", kind, times[call], 6 * n // 16, 16 * texels + 6 * n)
                modes = np.concatenate([bc6h_ref.block_modes(f.cpu().numpy().reshape(-1, 16)) for f in out])
                lines.append(f"{'':<28}modes: " + ", ".join(f"0x{m:02x} {100 * float((modes == m).mean()):.1f} %" for m in sorted(set(modes.tolist()))))
            lines.append(f"{'':<28}two-region time / one-region time: "
                         f"{statistics.median(times['..._ex TWO_REGION']) / statistics.median(times['pbr_bc6h_encode_cube']):.2f}")
            row("pbr_bc6h_decode_cube (of it)", f"{size}^2 x {mips}", kind, windows(lambda: ctx.bc6h_decode_cube(faces, size, mips, out=back)), 6 * n // 16,
                16 * texels + 6 * n)
        del cube, faces, faces2, back
        # pbr_bc1_encode at an equal block count: an S x 6 S RGBA8 chain
        w, h = size, 6 * size
        rgba8 = ctx.upload(rng.integers(0, 256, texture2d_bytes(w, h, mips, 28), dtype=np.uint8))
        blocks = ctx.bc1_encode(rgba8, w, h, mips, 28)[0]
        row("pbr_bc1_encode (scale)", f"{w}x{h} x {mips}", "random", windows(lambda: ctx.bc1_encode(rgba8, w, h, mips, 28, out=blocks)), blocks.numel() // 8,
            rgba8.numel() + blocks.numel())
        del rgba8, blocks
        torch.cuda.empty_cache()
    ctx.close()
    lines += ["", resource_usage(), ""] + quality_lines()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
