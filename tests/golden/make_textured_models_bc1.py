#!/usr/bin/env python3
"""Writes tests/golden/textured_models_bc1.npz: the maps of the reference scene's textured models (barrel, rock, suitcase, tile)
as the BC1 blocks their asset files hold, as DATA, for BC1-resident textures (PBR_TEX_BC1_BLOCKS) and pbr_bc1_decode.

Build container only (it reads the reference tree, make_sphere_grid.REF, which the GPU tests never see):

    python tests/golden/make_textured_models_bc1.py

The models, their materials and their texture files are found as tests/golden/make_textured_models.py finds them, and the
texture file's layout is the one described there: a TextureInfo header (uint16 width, height, depth, mips; uint8 DXGI format; 3
pad bytes), a uint32 byte count, then the BC1 blocks of every level (level i: max(1, ((w >> i) + 3) // 4) x max(1, ((h >> i) +
3) // 4) blocks of 8 bytes).  Nothing is decoded here.

Per map the file keeps the payload's bytes from the 128 x 128 level down (`{name}_{map}_blocks`, uint8) and `{name}_{map}_info`:
the original width, height, level count and format, then the kept chain's width, height and level count (the layout of
textured_models.npz's `_info`).  The 32 x 32 level and below are the levels textured_models.npz holds decoded: tests/test_bc1_cpu.py
checks the two against each other.  `name` and `maps` give the models and the map names in table order.  Meshes, matrices and
materials are not repeated: they are in textured_models.npz."""
import json
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(os.path.dirname(HERE))]
from make_sphere_grid import REF, load_json  # noqa: E402
from make_textured_models import MAPS  # noqa: E402

OUT = os.path.join(HERE, "textured_models_bc1.npz")
KEEP = 128                                    # the first level kept: 128 x 128 on the square assets


def read_blocks(rel):
    """the texture asset's BC1 payload from level KEEP down: (bytes, width, height, mips, format, kept width, height, levels)"""
    path = os.path.join(REF, rel.replace("\\", "/"))
    meta = json.load(open(os.path.splitext(path)[0] + ".json"))
    data = open(os.path.join(REF, meta["mTexturePath"].replace("\\", "/") + ".bin"), "rb").read()
    w, h, depth, mips, fmt = struct.unpack_from("<HHHHB", data, 0)
    nbytes = struct.unpack_from("<I", data, 12)[0]
    assert depth == 1 and 16 + nbytes == len(data), "unexpected texture layout"
    o, first = 16, None
    for l in range(mips):
        lw, lh = w >> l, h >> l
        if first is None and min(lw, lh) <= KEEP:
            first = (o, lw, lh, mips - l)
        o += max(1, (lw + 3) // 4) * max(1, (lh + 3) // 4) * 8
    assert o == len(data) and first is not None, "unexpected texture layout"
    return np.frombuffer(data[first[0]:], np.uint8), w, h, mips, fmt, first[1], first[2], first[3]


def main():
    doc = json.load(open(os.path.join(REF, "Asset/Scene/main.json")))
    out, names = {}, []
    for m in doc["mSceneModel"]:
        o = m["@SceneObject"]
        model = load_json(m["mModelFilePath"])
        mat = load_json(model["mMaterialPath"][0])
        if not mat.get("mTexturePath"):
            continue
        name = o["mName"]
        try:
            tex = {k: read_blocks(mat["mTexturePath"][key]) for k, key, flag in MAPS if mat["mParameterTable"].get(flag)}
        except FileNotFoundError:
            continue                          # (the revolver: listed as missing in textured_models.npz)
        names.append(name)
        for k, (blocks, w, h, mips, fmt, kw, kh, kl) in tex.items():
            out[f"{name}_{k}_blocks"] = blocks
            out[f"{name}_{k}_info"] = np.uint32([w, h, mips, fmt, kw, kh, kl])
    kept = [str(n) for n in np.load(os.path.join(HERE, "textured_models.npz"))["name"]]
    assert names == kept, (names, kept)      # the models textured_models.npz holds, in its order
    np.savez_compressed(OUT, name=np.array(names), maps=np.array([k for k, _, _ in MAPS]), **out)
    print(f"{OUT}: {names}, {sum(1 for k in out if k.endswith('_blocks'))} maps, "
          f"{sum(v.size for k, v in out.items() if k.endswith('_blocks'))} block bytes, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
