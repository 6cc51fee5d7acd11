#!/usr/bin/env python3
"""Times pbr_bc6h_decode_cube with HIP events on the context's stream after warm-up and writes profiles/bc6h_decode_ms.txt.

Rows: cubes of 512^2, 1024^2 and 2048^2 with their full chains, two kinds of input each:
  random   seeded random bytes: all 14 modes, the reserved codes and all partitions mixed in every wave (the kernel's worst case:
           a wave runs the header of every mode its lanes hold);
  smooth   blocks of one mode (0x03) made by the test-side encoder tests/bc6h_ref.encode_mode3 from the analytic sky of
           tests/golden/make_sky_bc6h.py: what a real sky looks like to the kernel, few modes per neighbourhood.  The encoder is numpy
           and slow, so a level larger than 128^2 repeats the 128^2 face's block grid; the timing sees the same mode and field mix.
Per row the median of three windows of --iters calls, the output rate (fp32 bytes written over that time) and the bytes moved (blocks
read + texels written) against the streaming rate measured in the same run (a device-to-device copy of 256 MiB, read + write bytes
over its time, as tools/texture_import_ms.py does).  Scale: pbr_bc1_decode of an RGBA8 chain with the same output byte count per
level (4 S x 6 S texels for a cube of edge S).  Also the upload bytes: the file against the fp32 chain.
Usage: python tools/bc6h_decode_ms.py [--iters N] [--sizes 512 1024 2048] [--out profiles/bc6h_decode_ms.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")]
HBM_PEAK = 8.0e12
SMOOTH_EDGE = 128


def smooth_faces(size, mips):
    """six mode-0x03 chains of a size^2 cube: per level the analytic sky at min(level edge, SMOOTH_EDGE) through encode_mode3, its
    block grid repeated to the level's"""
    import bc6h_ref
    from make_sky_bc6h import analytic_sky
    cache, faces = {}, [[] for _ in range(6)]
    for l in range(mips):
        s = size >> l
        e = min(s, SMOOTH_EDGE)
        if e not in cache:
            sky = analytic_sky(e)
            cache[e] = [bc6h_ref.encode_mode3(sky[f]) for f in range(6)]
        bw, be = bc6h_ref.level_blocks(s), bc6h_ref.level_blocks(e)
        for f in range(6):
            grid = cache[e][f].reshape(be, be, 16)
            faces[f].append(np.tile(grid, (bw // be, bw // be, 1)).reshape(-1))
    return [np.concatenate(f) for f in faces]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--sizes", type=int, nargs="*", default=[512, 1024, 2048])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bc6h_decode_ms.txt"))
    a = ap.parse_args()
    import bc6h_ref
    from direct12pbrrenderer_amd.api import PbrContext
    from direct12pbrrenderer_amd.structs import TEX_BC1_BLOCKS, bc6h_chain_bytes, cube_texels, texture2d_bytes
    from raster_ms import timed

    ctx = PbrContext(0)
    rng = np.random.default_rng(2026)

    def windows(fn):
        return [timed(fn, a.iters) for _ in range(3)]

    # the streaming rate of this device: a copy that reads and writes 256 MiB each
    src = ctx.empty((1 << 28,), torch.uint8)
    src.fill_(3)
    dst = torch.empty_like(src)
    copy_ms = statistics.median(windows(lambda: dst.copy_(src)))
    stream = 2.0 * src.numel() / (copy_ms * 1e-3)
    del src, dst
    torch.cuda.empty_cache()

    lines = [f"pbr_bc6h_decode_cube, {torch.cuda.get_device_name(0)}, HIP events on the context's stream, median of three windows of {a.iters} "
             "calls after 5 warm-up calls each",
             f"streaming rate measured here: device-to-device copy of 256 MiB, {copy_ms:.4f} ms -> {stream / 1e12:.2f} TB/s read + write "
             f"({100 * stream / HBM_PEAK:.0f} % of the 8 TB/s HBM peak; cubes up to 1024^2 fit the 256 MiB Infinity Cache, so repeated calls can run above it)",
             "out = fp32 RGBA bytes written (16 per texel); moved = blocks read + texels written; of stream = moved / time against the copy's rate",
             f"{'call':<26}{'cube / chain':>20}{'input':>9}{'ms':>10}{'out bytes':>12}{'out GB/s':>10}{'moved':>12}{'of stream':>11}   windows"]

    def row(call, what, kind, ms, out_bytes, in_bytes):
        med = statistics.median(ms)
        lines.append(f"{call:<26}{what:>20}{kind:>9}{med:>10.4f}{out_bytes:>12}{out_bytes / (med * 1e-3) / 1e9:>10.1f}{out_bytes + in_bytes:>12}"
                     f"{100 * (out_bytes + in_bytes) / (med * 1e-3) / stream:>10.1f}%   {' '.join(f'{t:.4f}' for t in ms)}")
        print(lines[-1], flush=True)

    uploads = []
    for size in a.sizes:
        mips = size.bit_length()
        n = bc6h_chain_bytes(size, mips)
        out_bytes = cube_texels(size, mips) * 16
        out = ctx.empty((cube_texels(size, mips), 4), torch.float32)
        inputs = {"random": [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(6)], "smooth": smooth_faces(size, mips)}
        assert all(f.size == n for f in inputs["smooth"]) and (bc6h_ref.block_modes(inputs["smooth"][0][:16 * 64]) == 3).all()
        for kind, faces in inputs.items():
            dev = [ctx.upload(f) for f in faces]
            row("pbr_bc6h_decode_cube", f"{size}^2 x {mips}", kind, windows(lambda: ctx.bc6h_decode_cube(dev, size, mips, out=out)), out_bytes, 6 * n)
            del dev
        del out
        # the scale: pbr_bc1_decode writing the same bytes per level (RGBA8, 4 S x 6 S)
        w, h = 4 * size, 6 * size
        assert texture2d_bytes(w, h, mips, 28) == out_bytes
        blocks = ctx.upload(rng.integers(0, 256, texture2d_bytes(w, h, mips, 28 | TEX_BC1_BLOCKS), dtype=np.uint8))
        dec = ctx.empty((out_bytes,), torch.uint8)
        row("pbr_bc1_decode (scale)", f"{w}x{h} x {mips}", "random", windows(lambda: ctx.bc1_decode(blocks, w, h, mips, 28, out=dec)), out_bytes, blocks.numel())
        del blocks, dec
        torch.cuda.empty_cache()
        uploads.append(f"upload, {size}^2 x {mips}: the file {6 * (16 + n) + 112} bytes, the fp32 chain {out_bytes} bytes ({out_bytes / (6 * (16 + n) + 112):.1f} x)")
    lines += [""] + uploads
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
