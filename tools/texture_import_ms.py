#!/usr/bin/env python3
"""Times the texture import path — pbr_texture2d_gen_mips and pbr_bc1_encode — with HIP events on the context's stream after warm-up
and writes profiles/texture_import_ms.txt.

Rows: one 2048^2 x 12 and one 1024^2 x 11 chain per stored format, and the whole 20-map table at the assets' sizes (the sizes,
level counts and stored formats of tests/golden/textured_models.npz's `_info`; seeded bytes).  Per row the median of three windows
of --iters calls, the bytes the call must move (gen_mips: level 0 read, levels 1.. written; encode: the chain read, the blocks
written) over that time, and that rate against the 8 TB/s HBM peak and against the streaming rate measured here (a device-to-device
copy of 256 MiB, read + write bytes over its time).  pbr_bc1_decode of the same table is the scale, scene.mip_chain and the numpy
restatement of the encoder (tests/bc1_encode_ref.py) the host legs.
Also: the encoder's quality per level against the yardstick fixture (CPU, the restatement: the GPU equals it bit for bit), and the
share of G-buffer bytes that BC1 import changes in the reference scene at 1440 x 960.

--parent-runs / --this-runs: output files (--out, named <tool>_<run>.txt) of tools/raster_tex_ms.py and tools/raster_bc1_ms.py from
alternating runs of the parent commit's and this commit's tree in one session: the existing raster rows (constant-only, textured,
decoded-resident, BC1-resident) against the parent's spread are appended.
Usage: python tools/texture_import_ms.py [--iters N] [--out profiles/texture_import_ms.txt] [--parent-runs F... --this-runs F...]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
HBM_PEAK = 8.0e12


RASTER_ROWS = ("constant-only", "textured", "decoded-resident", "BC1-resident")


def raster_rows(path):
    """{(row, size): raster ms} of one output file of tools/raster_tex_ms.py or tools/raster_bc1_ms.py"""
    rows = {}
    for line in open(path):
        f = line.split()
        if len(f) >= 4 and f[0] in RASTER_ROWS and "x" in f[1]:
            rows[(f[0], f[1])] = float(f[3])
    return rows


def regression_lines(parent_files, this_files):
    """the existing raster rows: every (row, size) that occurs in the parent's files, the parent's spread against itself and the
    difference of the medians; the files of one side are merged run by run (file names sort as run 1, 2, 3 per tool)"""
    def merged(files):
        by_tool = {}
        for p in files:
            by_tool.setdefault(os.path.basename(p).rsplit("_", 1)[0], []).append(raster_rows(p))
        runs = max(len(v) for v in by_tool.values())
        return [{k: v for tool in by_tool.values() if r < len(tool) for k, v in tool[r].items()} for r in range(runs)]
    parent, this = merged(parent_files), merged(this_files)
    lines = ["", f"existing raster rows, tools/raster_tex_ms.py and tools/raster_bc1_ms.py of the parent commit and of this commit run alternately in one "
             f"session ({len(parent)} + {len(this)} runs), raster ms:",
             f"{'row':<18}{'size':>11}  {'parent runs':<26}{'this commit runs':<26}{'parent max-min':>15}{'median diff':>13}  verdict"]
    for key in sorted(parent[0], key=lambda k: (int(k[1].split("x")[0]), RASTER_ROWS.index(k[0]))):
        p, t = [r[key] for r in parent if key in r], [r[key] for r in this if key in r]
        spread, diff = max(p) - min(p), statistics.median(t) - statistics.median(p)
        lines.append(f"{key[0]:<18}{key[1]:>11}  {' '.join(f'{x:.4f}' for x in p):<26}{' '.join(f'{x:.4f}' for x in t):<26}{spread:>15.4f}"
                     f"{diff:>+13.4f}  {'within the spread' if diff <= spread else 'SLOWER THAN THE SPREAD'}")
    return lines


def bound_lines(medians, stream, blocks_2048):
    """which bound each call sits on, decided from the measured rows: how the time follows the bytes (4-byte against 1-byte texels at
    one size: 4 x the bytes in, the same work per texel or block; 2048^2 against 1024^2: 4 x both) and the rate against the
    streaming rate.  A call whose time follows neither is at its launch floor."""
    lines = []
    for call, unit in (("pbr_texture2d_gen_mips", "texels"), ("pbr_bc1_encode", "blocks")):
        t28, b28 = medians[(call, "2048^2 x 12", 28)]
        t61, b61 = medians[(call, "2048^2 x 12", 61)]
        t1k, _ = medians[(call, "1024^2 x 11", 28)]
        t8k, b8k = medians[(call, "8192^2 x 14", 28)]
        by_bytes, by_work, of_stream = t28 / t61, t28 / t1k, b8k / (t8k * 1e-3) / stream
        if by_work < 1.5 and by_bytes < 1.5:
            verdict = (f"at 2048^2 and below the time follows neither the bytes nor the {unit}: the floor of the call's launches, not a bound of the device")
        elif by_bytes >= 2.0:
            verdict = "the time follows the bytes: HBM / cache bandwidth"
        else:
            verdict = f"the time follows the {unit} ({by_work:.2f} x for 4 x) and not the bytes ({by_bytes:.2f} x for {b28 / b61:.1f} x): instruction issue (VALU), not HBM"
        big = "HBM" if of_stream >= 0.5 else "below the streaming rate: not HBM at this size either"
        lines.append(f"bound, {call}: 2048^2 x 12 format 28 {t28:.4f} ms, format 61 {t61:.4f} ms ({b28 / b61:.1f} x fewer bytes, time ratio {by_bytes:.2f}); "
                     f"1024^2 x 11 format 28 {t1k:.4f} ms (4 x fewer {unit}, time ratio {by_work:.2f}) -> {verdict}; 8192^2 x 14 (out of cache) {t8k:.4f} ms = "
                     f"{100 * of_stream:.1f} % of the streaming rate -> {big}")
    t28, _ = medians[("pbr_bc1_encode", "2048^2 x 12", 28)]
    lines.append(f"pbr_bc1_encode, 2048^2 x 12: {blocks_2048} blocks, {blocks_2048 / (t28 * 1e-3) / 1e9:.2f} G blocks/s")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_import_ms.txt"))
    ap.add_argument("--parent-runs", nargs="*", default=[])
    ap.add_argument("--this-runs", nargs="*", default=[])
    a = ap.parse_args()
    import bc1_encode_ref
    from direct12pbrrenderer_amd import scene
    from direct12pbrrenderer_amd.api import PbrContext
    from direct12pbrrenderer_amd.structs import TEX_BC1_BLOCKS, Tile, texture2d_bytes
    from raster_ms import timed
    from test_texture_import_cpu import GOLDEN, fixture_images

    ctx = PbrContext(0)
    rng = np.random.default_rng(2025)
    fxt = np.load(os.path.join(ROOT, "tests", "golden", "textured_models.npz"))
    infos = [tuple(int(x) for x in fxt[f"{n}_{k}_info"][:4]) for n in fxt["name"] for k in fxt["maps"] if f"{n}_{k}_info" in fxt.files]

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

    def chain(w, h, mips, fmt):
        """a chain-sized device buffer with seeded level-0 bytes and its generated levels; and its block buffer"""
        n = texture2d_bytes(w, h, mips, fmt)
        texel = 1 if fmt == 61 else 4
        dev = ctx.empty((n,), torch.uint8)
        dev[:w * h * texel].copy_(torch.from_numpy(rng.integers(0, 256, w * h * texel, dtype=np.uint8)))
        ctx.texture2d_gen_mips(dev, w, h, mips, fmt)
        return dev, ctx.empty((texture2d_bytes(w, h, mips, fmt | TEX_BC1_BLOCKS),), torch.uint8)

    lines = [f"pbr_texture2d_gen_mips and pbr_bc1_encode, {torch.cuda.get_device_name(0)}, HIP events on the context's stream, median of three "
             f"windows of {a.iters} calls after 5 warm-up calls each; seeded random bytes",
             f"streaming rate measured here: device-to-device copy of 256 MiB, {copy_ms:.4f} ms -> {stream / 1e12:.2f} TB/s read + write "
             f"({100 * stream / HBM_PEAK:.0f} % of the 8 TB/s HBM peak; the 2048^2 chains fit the 256 MiB Infinity Cache, so repeated calls on one "
             "chain can run above it)",
             "bytes = what the call must move: gen_mips reads level 0 and writes levels 1..; encode reads the chain and writes the blocks",
             f"{'call':<24}{'chain':>16}{'format':>8}{'ms':>10}{'bytes':>12}{'GB/s':>9}{'of peak':>9}{'of stream':>11}   windows"]

    medians = {}

    def row(call, what, fmt, ms, nbytes):
        rate = nbytes / (statistics.median(ms) * 1e-3)
        medians[(call, what, fmt)] = (statistics.median(ms), nbytes)
        lines.append(f"{call:<24}{what:>16}{fmt:>8}{statistics.median(ms):>10.4f}{nbytes:>12}{rate / 1e9:>9.1f}{100 * rate / HBM_PEAK:>8.1f}%"
                     f"{100 * rate / stream:>10.1f}%   {' '.join(f'{t:.4f}' for t in ms)}")
        print(lines[-1], flush=True)

    for w, mips, fmts in ((2048, 12, (28, 87, 91, 61)), (1024, 11, (28, 87, 91, 61)), (8192, 14, (28,))):   # (8192^2: larger than the caches)
        for fmt in fmts:
            dev, blocks = chain(w, w, mips, fmt)
            n = texture2d_bytes(w, w, mips, fmt)
            row("pbr_texture2d_gen_mips", f"{w}^2 x {mips}", fmt, windows(lambda: ctx.texture2d_gen_mips(dev, w, w, mips, fmt)), n)
            row("pbr_bc1_encode", f"{w}^2 x {mips}", fmt, windows(lambda: ctx.bc1_encode(dev, w, w, mips, fmt, out=blocks)), n + blocks.numel())
            del dev, blocks
    table = [chain(w0, h0, m0, fmt) for w0, h0, m0, fmt in infos]
    bytes_dec = sum(texture2d_bytes(*inf) for inf in infos)
    bytes_bc1 = sum(b.numel() for _, b in table)
    what = f"{len(infos)} maps"

    def mips_all():
        for (dev, _), (w0, h0, m0, fmt) in zip(table, infos):
            ctx.texture2d_gen_mips(dev, w0, h0, m0, fmt)

    def encode_all():
        for (dev, blocks), (w0, h0, m0, fmt) in zip(table, infos):
            ctx.bc1_encode(dev, w0, h0, m0, fmt, out=blocks)

    def decode_all():
        for (dev, blocks), (w0, h0, m0, fmt) in zip(table, infos):
            ctx.bc1_decode(blocks, w0, h0, m0, fmt, out=dev)
    row("pbr_texture2d_gen_mips", what, "all", windows(mips_all), bytes_dec)
    row("pbr_bc1_encode", what, "all", windows(encode_all), bytes_dec + bytes_bc1)
    row("pbr_bc1_decode (scale)", what, "all", windows(decode_all), bytes_dec + bytes_bc1)
    lines.append(f"the table: {len(infos)} chains, {sum(w0 * h0 for w0, h0, _, _ in infos)} level-0 texels, {bytes_dec} bytes uncompressed, {bytes_bc1} bytes as BC1")
    del table
    torch.cuda.empty_cache()
    lines += bound_lines(medians, stream, texture2d_bytes(2048, 2048, 12, 28 | TEX_BC1_BLOCKS) // 8)

    # the host legs (one run each, wall clock): what the GPU path replaces
    lv0 = rng.integers(0, 256, (2048, 2048, 4), dtype=np.uint8)
    t0 = time.perf_counter()
    levels = scene.mip_chain(lv0)
    t_mips = time.perf_counter() - t0
    t0 = time.perf_counter()
    bc1_encode_ref.encode_level(levels[1], 28)
    t_enc = time.perf_counter() - t0
    lines += ["", f"host legs on this machine's CPU (one run, wall clock): scene.mip_chain of 2048^2 x 12 RGBA {1e3 * t_mips:.1f} ms; "
              f"tests/bc1_encode_ref.py (numpy) of one 1024^2 level {1e3 * t_enc:.1f} ms ({1024 * 1024 / t_enc / 1e6:.2f} M texels/s)"]

    # quality per level against the yardstick (the restatement on the CPU; the GPU's blocks equal it bit for bit: tests)
    y = np.load(os.path.join(GOLDEN, "bc1_encode_yardstick.npz"))
    lines += ["", "encoder quality under the pinned decode, total squared error over r, g, b per level, against Pillow's DXT1 blocks "
              "(tests/golden/bc1_encode_yardstick.npz); level 0 = decodes of the assets' own blocks, levels 1-3 = box-filtered",
              f"{'map':<20}" + "".join(f"{f'l{l} own':>11}{f'l{l} Pillow':>11}" for l in range(4))]
    sums = np.zeros((4, 2), np.int64)
    worse = []
    for n, k, _, rgb in fixture_images():
        cells = ""
        for l, img in enumerate(scene.mip_chain(rgb, 4)):
            own = bc1_encode_ref.squared_error(bc1_encode_ref.encode_rgb(img), img)
            pil = bc1_encode_ref.squared_error(y[f"{n}_{k}_l{l}"], img)
            sums[l] += (own, pil)
            if own > pil:
                worse.append(f"{n} {k} level {l} ({10 * np.log10(own / pil):.2f} dB)")
            cells += f"{own:>11}{pil:>11}"
        lines.append(f"{n + ' ' + k:<20}" + cells)
    lines.append(f"{'sum':<20}" + "".join(f"{int(s[0]):>11}{int(s[1]):>11}" for s in sums))
    lines.append(f"levels 1-3 summed: {int(sums[1:, 0].sum())} against Pillow's {int(sums[1:, 1].sum())} "
                 f"({sums[1:, 0].sum() / sums[1:, 1].sum():.2f} x); above Pillow's error on: {', '.join(worse) if worse else 'none'}")

    # BC1 import in the reference scene: how many G-buffer bytes differ from the uncompressed import
    from oracle import binding as orc
    from test_gpu_raster_tex import gpu_raster_tex, reference_textured_scene
    w, h = 1440, 960
    g, v, i, d, maps, texs, _, _, _ = reference_textured_scene(w, h, orc)
    tile = Tile(0, 0, w, h, w, h)
    planes = {}
    for bc1 in (False, True):
        pairs = scene.import_texture_table(ctx, texs, bc1=bc1)
        planes[bc1] = gpu_raster_tex(ctx, g, tile, v, i, d, maps, [], descs=[p[1] for p in pairs])
    differing = sum(int((planes[True][k].view(np.uint8) != planes[False][k].view(np.uint8)).sum()) for k in ("A", "B", "C"))
    lines += ["", f"reference scene at {w}x{h}, the 20 maps (32 x 32 level 0 of the fixture) through import_texture: with bc1=True {differing} of "
              f"{12 * w * h} A/B/C bytes differ from the uncompressed import ({100.0 * differing / (12 * w * h):.3f} %)"]
    ctx.close()
    if a.parent_runs and a.this_runs:
        lines += regression_lines(a.parent_runs, a.this_runs)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
