#!/usr/bin/env python3
"""Writes tests/golden/bc1_encode_yardstick.npz: a third-party BC1 encoder's blocks, as DATA, for the quality conditions of
pbr_bc1_encode (tests/test_texture_import_cpu.py).

Build container only (needs Pillow, which the tests never import):

    python tests/golden/make_bc1_encode_yardstick.py

For each of the 20 chains of tests/golden/textured_models_bc1.npz: its level 0 (128 x 128), decoded by tests/bc1_ref.py and read as
R, G, B whatever format the chain is stored in, and the levels 1 .. 3 that scene.mip_chain makes from that image (64, 32 and 16
texels square), each encoded by Pillow's DDS writer (Image.save(buf, "DDS", pixel_format="DXT1"); the payload starts at byte 128 of
the file).  Kept per chain: `{name}_{map}_l{level}` (uint8, the blocks of that level).  `name` and `maps` repeat the BC1 fixture's;
`levels` is the number of levels kept.  The level-0 images are decodes of blocks DirectXTex wrote, so an ideal encoder reproduces
them exactly; the box-filtered levels are not BC1-representable."""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import bc1_ref  # noqa: E402
from direct12pbrrenderer_amd import scene  # noqa: E402

OUT = os.path.join(HERE, "bc1_encode_yardstick.npz")
LEVELS = 4


def images(fxb):
    """(model, map, the LEVELS [h, w, 3] uint8 images of the chain) in table order"""
    for n in (str(x) for x in fxb["name"]):
        for k in (str(x) for x in fxb["maps"]):
            if f"{n}_{k}_blocks" not in fxb.files:
                continue
            _, _, _, _, w, h, _ = (int(x) for x in fxb[f"{n}_{k}_info"])
            bw, bh = bc1_ref.level_blocks(w, h)
            rgb = np.ascontiguousarray(bc1_ref.decode_level(fxb[f"{n}_{k}_blocks"][:8 * bw * bh], w, h)[..., :3])
            yield n, k, scene.mip_chain(rgb, LEVELS)


def pillow_blocks(rgb):
    h, w, _ = rgb.shape
    buf = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(buf, "DDS", pixel_format="DXT1")
    blocks = np.frombuffer(buf.getvalue()[128:], np.uint8)
    assert blocks.size == 8 * (w // 4) * (h // 4)
    return blocks


def main():
    fxb = np.load(os.path.join(HERE, "textured_models_bc1.npz"))
    out = {}
    for n, k, levels in images(fxb):
        for l, rgb in enumerate(levels):
            out[f"{n}_{k}_l{l}"] = pillow_blocks(rgb)
    np.savez_compressed(OUT, name=fxb["name"], maps=fxb["maps"], levels=np.uint32(LEVELS), **out)
    print(f"{OUT}: {len(out)} levels, {sum(v.size for v in out.values())} block bytes, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
