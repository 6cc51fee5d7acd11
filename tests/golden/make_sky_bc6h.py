#!/usr/bin/env python3
"""Writes tests/golden/sky_bc6h.npz: two sky cubes in the reference's serialized cube-map layout (six BC6H_UF16 chains + the SH pack;
direct12pbrrenderer_amd/host/CubeMapFile.h), as DATA, for pbr_bc6h_decode_cube and pbrh_set_skybox_file.

    python tests/golden/make_sky_bc6h.py          (needs the built host library and the oracle; no GPU, nothing of the reference)

`smooth_file` (uint8): a 32^2 cube with its full chain of six levels.  Level 0 is an analytic sky — the gradient and sun lobe of
synth.env_cube without its noise, the sun reaching about 50 — and every level is its 2 x 2 box mip, encoded by the test-side
single-mode encoder tests/bc6h_ref.encode_mode3.  Its SH pack is the oracle's projection (orc.sh9_project) of the DECODED level 0,
what a reference import would have stored beside the blocks.
`random_file` (uint8): a 16^2 cube with its full chain of five levels whose blocks are seeded random bytes (every mode, partition
and reserved code mixed); its SH pack is 28 seeded floats (random blocks decode to values up to 65504: a projection says nothing).
`smooth_level0` (float32 [6, 32, 32, 3]): the analytic level 0 before encoding, for the encoder's sanity test."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.dirname(HERE), ROOT]
import bc6h_ref  # noqa: E402
from direct12pbrrenderer_amd import host, synth  # noqa: E402
from oracle import binding as orc  # noqa: E402

OUT = os.path.join(HERE, "sky_bc6h.npz")
SMOOTH_SIZE, SMOOTH_MIPS = 32, 6
RANDOM_SIZE, RANDOM_MIPS = 16, 5


def analytic_sky(size):
    """float32 [6, size, size, 3]: (0.3, 0.5, 0.9) (0.5 + 0.5 d.y) + 50 exp(-200 (1 - d.s)), s = (1, 1, 1) / sqrt 3"""
    d = synth.cube_directions(size)
    s = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    rgb = np.array([0.3, 0.5, 0.9])[None, None, None, :] * (0.5 + 0.5 * d[..., 1])[..., None] + (50.0 * np.exp(-200.0 * (1.0 - d @ s)))[..., None]
    return rgb.astype(np.float32)


def main():
    level0 = analytic_sky(SMOOTH_SIZE)
    assert level0.max() > 10.0
    faces = [bc6h_ref.encode_mode3_chain(level0[f], SMOOTH_MIPS) for f in range(6)]
    decoded = bc6h_ref.decode_cube(faces, SMOOTH_SIZE, SMOOTH_MIPS)
    sh = orc.sh9_project(np.ascontiguousarray(decoded[:6 * SMOOTH_SIZE ** 2]).reshape(-1), SMOOTH_SIZE)
    smooth = host.write_cubemap_file(faces, SMOOTH_SIZE, SMOOTH_MIPS, sh)
    rng = np.random.default_rng(0xBC6)
    n = bc6h_ref.chain_bytes(RANDOM_SIZE, RANDOM_MIPS)
    random = host.write_cubemap_file([rng.integers(0, 256, n, dtype=np.uint8) for _ in range(6)], RANDOM_SIZE, RANDOM_MIPS,
                                     rng.standard_normal(28).astype(np.float32))
    np.savez_compressed(OUT, smooth_file=np.frombuffer(smooth, np.uint8), random_file=np.frombuffer(random, np.uint8), smooth_level0=level0)
    print(f"{OUT}: smooth {len(smooth)} B, random {len(random)} B, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
