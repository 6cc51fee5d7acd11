"""The resident BC6H sky on the CPU (include/pbr_hip.h: pbr_skybox_bc6h): the per-texel decode the kernel runs
(csrc/bc6h_decode_block.hpp) compiled for the host in a stand-alone program under ASan / UBSan against the numpy restatement
(tests/bc6h_ref.py), the ctypes declaration against the header's argument list, and the conditions the GPU test's inputs have to meet
(tests/sky_bc6h_cases.py).  No GPU; reads tests/golden/ only."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bc6h_ref
import sky_bc6h_cases as cases
from direct12pbrrenderer_amd import _lib, host, structs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(HERE, "golden", "sky_bc6h.npz"), allow_pickle=False))


def test_per_texel_decode_on_the_host_under_sanitizers(fixture, tmp_path):
    """csrc/bc6h_decode_block.hpp — header() and texel(), the text k_skybox_bc6h runs per block and per tap — compiled for the host with
    -fsanitize=address,undefined in a program of its own (tools/bc6h_texel_hostcheck.cpp; every face in a buffer of exactly its chain's
    bytes): every texel of the 4^2 x 3, 12^2 x 4 and 32^2 x 6 random-block cubes and of the two fixture files equals
    bc6h_ref.decode_cube as a uint32, and the sanitizers report nothing"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler builds the oracle and the host library: it must be there"
    exe = tmp_path / "bc6h_texel_hostcheck"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                    "-o", str(exe), os.path.join(ROOT, "tools", "bc6h_texel_hostcheck.cpp")], check=True)
    cubes = {f"random {s}^2 x {m}": (s, m, cases.random_faces(s, m)) for s, m in ((4, 3), (12, 4), (32, 6))}
    for name in ("smooth_file", "random_file"):
        data = fixture[name]
        size, mips, offsets, _ = host.parse_cubemap_file(data.tobytes())
        n = bc6h_ref.chain_bytes(size, mips)
        cubes[name] = (size, mips, [data[o:o + n] for o in offsets])
    modes = set()
    for name, (size, mips, faces) in cubes.items():
        (tmp_path / "in.bin").write_bytes(np.uint32([size, mips]).tobytes() + b"".join(np.asarray(f, np.uint8).tobytes() for f in faces))
        run = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
        assert run.returncode == 0 and not run.stderr, (name, run.stderr[-2000:])
        got = np.fromfile(tmp_path / "out.bin", np.uint32).reshape(-1, 4)
        want = bc6h_ref.decode_cube(faces, size, mips).view(np.uint32)
        assert got.shape == want.shape == (structs.cube_texels(size, mips), 4), name
        assert np.array_equal(got, want), (name, int((got != want).any(axis=1).sum()))
        modes |= set(np.concatenate([bc6h_ref.block_modes(f) for f in faces]).tolist())
    assert modes >= set(bc6h_ref.MODES) | set(bc6h_ref.RESERVED)          # every mode and every reserved code went through it


def test_ctypes_declaration_matches_the_header():
    """_lib.py declares pbr_skybox_bc6h with the header's argument list, CubeBc6h mirrors pbr_cube_bc6h, and the libraries export the
    new entry points"""
    text = open(os.path.join(ROOT, "include", "pbr_hip.h")).read()
    m = re.search(r"pbr_status\s+pbr_skybox_bc6h\s*\(([^;]*)\)\s*;", text)
    assert m, "pbr_skybox_bc6h is not declared in include/pbr_hip.h"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert [re.sub(r"\s*\w+$", "", a) for a in args] == ["pbr_ctx*", "const pbr_global*", "const pbr_tile*", "const pbr_cube_bc6h*",
                                                         "const uint8_t*", "uint32_t", "pbr_half*", "uint32_t"], args
    res, argtypes = _lib.SIGNATURES["pbr_skybox_bc6h"]
    assert res is C.c_int
    assert argtypes == [C.c_void_p, C.POINTER(structs.Global), C.POINTER(structs.Tile), C.POINTER(structs.CubeBc6h), C.c_void_p, C.c_uint32,
                        C.c_void_p, C.c_uint32]
    # the same list as pbr_skybox's but for the cube
    assert [a for i, a in enumerate(argtypes) if i != 3] == [a for i, a in enumerate(_lib.SIGNATURES["pbr_skybox"][1]) if i != 3]
    s = re.search(r"typedef struct pbr_cube_bc6h \{([^}]*)\}", text)
    assert s and re.sub(r"\s+", " ", s.group(1)).strip() == "const void* face_blocks[6]; uint32_t size, mips;"
    assert [f[0] for f in structs.CubeBc6h._fields_] == ["face_blocks", "size", "mips"]
    assert C.sizeof(structs.CubeBc6h) == 6 * C.sizeof(C.c_void_p) + 8 and structs.CubeBc6h.size.offset == 6 * C.sizeof(C.c_void_p)
    assert _lib.load().pbr_skybox_bc6h
    lib = host.load()
    assert lib.pbrh_set_skybox_file_resident and lib.pbrh_load_skybox_file_resident and lib.pbrh_sky_resident_bytes


def test_the_gpu_cases_cover_what_the_kernel_can_get_wrong():
    """the inputs of tests/test_gpu_sky_bc6h.py, analysed in float64 (camera_ref's rays and faces, the kernel's LOD formula): centre rays
    on all six faces; every level of the 8^2 x 4 and the 12^2 x 4 chain — the 2- and 1-texel levels too — is the lower level of some sky
    pixel; fractional LODs and LOD 0 both occur; 96 x 64 on the size-4 cube keeps most footprints in one block; the minified case holds
    footprints of one, two and four blocks, a seam gives three; and the camera aimed at a block corner puts most footprints in four
    blocks (a footprint is 2 x 2 adjacent texels of its level at any LOD, so inside a face only one pixel position in sixteen straddles
    a corner: see sky_bc6h_cases)"""
    cases.assert_coverage(cases.coverage())
    for cube in cases.CUBES:
        assert bc6h_ref.chain_bytes(*cube) == structs.bc6h_chain_bytes(*cube) > 0
    assert cases.RAGGED == (200, 37, (640, 360), 328, 91)
