#!/usr/bin/env python3
"""Times the sky pass on a sky resident as BC6H_UF16 blocks (pbr_skybox_bc6h) against the same pass on the decoded fp32 cube
(pbr_skybox on pbr_bc6h_decode_cube's output), alternated in one run, and writes profiles/skybox_bc6h_ms.txt.

Frames: 1440x960 and 3840x2160, stencil all zero (every pixel is sky), the reference's default camera.
Cubes: 2048^2 x 12 and 512^2 x 10, two kinds of content each:
  synth    synth.env_cube's 512^2 sky (gradient, sun lobe, 5 % noise; above 512^2 the faces are tiled), box mips from
           pbr_cube_gen_mips, compressed by pbr_bc6h_encode_cube: the importer's files, four one-region modes;
  synth2   the same cube compressed with PBR_BC6H_ENCODE_TWO_REGION: the importer's files with the flag, the mode mix of a real
           two-region encoder;
  random   seeded random bytes: every mode, partition and reserved code in every wave — the worst case for a kernel that runs every
           mode header its wave holds.
Per row the median of three windows of --iters calls (HIP events, 5 warm-up calls per window), the two targets compared bit for bit
before anything is timed, the resident bytes of both forms, and the device-to-device copy rate of the same run.  Then the new
kernel's register, occupancy and scratch figures as the compiler reports them.  There is no pass mark on time.
Usage: python tools/skybox_bc6h_ms.py [--iters N] [--out profiles/skybox_bc6h_ms.txt]"""
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
HBM_PEAK = 8.0e12
SYNTH_EDGE = 512


def resource_usage():
    """k_skybox_bc6h's figures from -Rpass-analysis=kernel-resource-usage (a compile of the one translation unit, nothing is kept)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return "kernel resource usage: not measured (no hipcc here)"
    src = os.path.join(ROOT, "direct12pbrrenderer_amd", "csrc", "raster.hip")
    with tempfile.TemporaryDirectory() as tmp:
        run = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                              "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "x.o")], capture_output=True, text=True)
    out, kernel, got = [], None, {}

    def flush():
        if kernel and "VGPRs" in got:
            out.append(f"{kernel}, gfx950 (-Rpass-analysis=kernel-resource-usage): VGPRs {got.get('VGPRs')}, SGPRs {got.get('TotalSGPRs')}, occupancy "
                       f"{got.get('Occupancy')} waves/SIMD, scratch {got.get('ScratchSize')} bytes/lane, VGPR spills {got.get('VGPRs Spill')}, LDS "
                       f"{got.get('LDS Size')} bytes/block")
    for line in run.stderr.splitlines():                      # (the compiler prints source excerpts between the remarks)
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            flush()
            name = m.group(1)
            kernel, got = ("k_skybox_bc6h" if "k_skybox_bc6h" in name else "k_skybox" if "k_skybox" in name else None), {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if m and kernel:
            got[m.group(1)] = m.group(2)
    flush()
    return "\n".join(out) if out else "kernel resource usage: not measured (the compile reported nothing)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skybox_bc6h_ms.txt"))
    ap.add_argument("--cubes", default="2048x12,512x10")
    ap.add_argument("--sizes", default="1440x960,3840x2160")
    a = ap.parse_args()
    import bc6h_ref
    from direct12pbrrenderer_amd import scene, synth
    from direct12pbrrenderer_amd.api import PbrContext
    from direct12pbrrenderer_amd.structs import Tile, bc6h_chain_bytes, cube_texels
    from raster_ms import timed

    ctx = PbrContext(0)
    rng = np.random.default_rng(2027)
    src = ctx.empty((1 << 28,), torch.uint8)
    src.fill_(3)
    dst = torch.empty_like(src)
    copy_ms = statistics.median([timed(lambda: dst.copy_(src), 50) for _ in range(3)])
    stream = 2.0 * src.numel() / (copy_ms * 1e-3)
    del src, dst
    torch.cuda.empty_cache()

    lines = [f"pbr_skybox_bc6h (BC6H-resident sky, sampled in place) against pbr_skybox on the decoded fp32 cube, {torch.cuda.get_device_name(0)}, HIP "
             f"events, median of three alternated windows of {a.iters} calls after 5 warm-up calls each; stencil all zero; the two targets are "
             "equal bit for bit (checked before timing)",
             f"streaming rate measured here: device-to-device copy of 256 MiB, {copy_ms:.4f} ms -> {stream / 1e12:.2f} TB/s read + write "
             f"({100 * stream / HBM_PEAK:.0f} % of the 8 TB/s HBM peak)",
             "target bytes = the 8-byte HDR store + the stencil byte per pixel; of copy = target bytes / time against the copy's rate",
             f"{'cube':<12}{'content':<9}{'frame':>11}{'row':>10}{'ms':>10}{'resident bytes':>16}{'of copy':>9}{'ratio':>8}   windows"]
    synth0 = torch.from_numpy(synth.env_cube(SYNTH_EDGE, 1).reshape(6, SYNTH_EDGE, SYNTH_EDGE, 4))
    for size, mips in (tuple(int(x) for x in c.split("x")) for c in a.cubes.split(",")):
        n = bc6h_chain_bytes(size, mips)
        texels = cube_texels(size, mips)
        for content in ("synth", "synth2", "random"):
            if content != "random":
                cube = ctx.empty((texels, 4), torch.float32)
                e = min(size, SYNTH_EDGE)
                lv = synth0 if e == SYNTH_EDGE else torch.from_numpy(synth.env_cube(e, 1).reshape(6, e, e, 4))
                cube[:6 * size * size].copy_(lv.repeat(1, size // e, size // e, 1).reshape(-1, 4))
                ctx.cube_gen_mips(cube, size, mips)
                faces = ctx.bc6h_encode_cube(cube, size, mips, two_region=content == "synth2")
                ctx.sync()
                del cube
            else:
                faces = [ctx.upload(rng.integers(0, 256, n, dtype=np.uint8)) for _ in range(6)]
            modes = np.concatenate([bc6h_ref.block_modes(f[:16 * 65536].cpu().numpy().reshape(-1, 16)) for f in faces])
            decoded = ctx.bc6h_decode_cube(faces, size, mips)
            ctx.sync()
            lines.append(f"{f'{size}^2 x {mips}':<12}{content:<9}modes of the first 64 Ki blocks of each face: "
                         + ", ".join(f"0x{m:02x} {100 * float((modes == m).mean()):.1f} %" for m in sorted(set(modes.tolist()))[:18]))
            for w, h in (tuple(int(x) for x in s.split("x")) for s in a.sizes.split(",")):
                g = scene.make_global(scene.Camera.reference_default(w, h), w, h)
                tile = Tile(0, 0, w, h, w, h)
                sten = ctx.zeros((h, w), torch.uint8)
                hdr_a, hdr_b = ctx.zeros((h, w, 4), torch.float16), ctx.zeros((h, w, 4), torch.float16)
                rows = {"decoded": lambda: ctx.skybox(g, tile, decoded, size, mips, sten, w, hdr_a, w),
                        "resident": lambda: ctx.skybox_bc6h(g, tile, faces, size, mips, sten, w, hdr_b, w)}
                for fn in rows.values():
                    fn()
                ctx.sync()
                assert torch.equal(hdr_a.view(torch.int16), hdr_b.view(torch.int16)), f"{size} {content} {w}x{h}: the targets differ"
                times = {row: [] for row in rows}
                for _ in range(3):                                # the rows alternate: three timed windows each
                    for row, fn in rows.items():
                        times[row].append(timed(fn, a.iters))
                base = statistics.median(times["decoded"])
                for row in rows:
                    med = statistics.median(times[row])
                    nbytes = 16 * texels if row == "decoded" else 6 * n
                    lines.append(f"{f'{size}^2 x {mips}':<12}{content:<9}{f'{w}x{h}':>11}{row:>10}{med:>10.4f}{nbytes:>16}"
                                 f"{100 * 9 * w * h / (med * 1e-3) / stream:>8.2f}%{med / base:>8.3f}   {' '.join(f'{t:.4f}' for t in times[row])}")
                    print(lines[-1], flush=True)
                del sten, hdr_a, hdr_b
            del faces, decoded
            torch.cuda.empty_cache()
    ctx.close()
    lines += ["", resource_usage()]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
