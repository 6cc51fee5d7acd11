"""The chain geometry every texture entry point shares (csrc/tex_chain.hpp: levels, offsets, block counts, refusals, the level tables
of the lane = block kernels) compiled for the host in a stand-alone program under ASan / UBSan (tools/tex_chain_hostcheck.cpp) and
held to the Python restatements, which keep their own arithmetic: structs.texture2d_bytes / bc6h_chain_bytes / cube_mip_offset,
tests/bc1_ref.py and tests/bc6h_ref.py.  No GPU."""
import os
import shutil
import subprocess

import pytest

import bc1_ref
import bc6h_ref
from direct12pbrrenderer_amd import structs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

STORED = (structs.TEX_R8G8B8A8_UNORM, structs.TEX_B8G8R8A8_UNORM, structs.TEX_B8G8R8A8_UNORM_SRGB, structs.TEX_R8_UNORM)
BC1 = structs.TEX_BC1_BLOCKS
# width, height, levels.  4097 x 4 lies inside PBR_TEX_MAX_SIZE = 16384 and is accepted, as it always was; one above the limit is
# 16385.  The largest chain (16384^2 x 15) fills every entry of the table.
ACCEPTED_2D = [(1, 1, 1), (4, 4, 3), (5, 3, 2), (7, 9, 3), (20, 12, 3), (9, 5, 3), (64, 16, 5), (4096, 1, 1), (4097, 4, 1),
               (4096, 4096, 13), (16384, 1, 1), (16384, 16384, 15)]
REFUSED_2D = [(0, 4, 1, "size"), (4, 0, 1, "size"), (16385, 4, 1, "size"), (4, 16385, 1, "size"), (8, 8, 5, "mip_levels"), (8, 8, 0, "mip_levels")]
BAD_FORMATS = [29, 0, structs.TEX_R8G8B8A8_UNORM | 0x200, structs.TEX_R8_UNORM | 0x10000, structs.TEX_R8_UNORM | BC1 | 0x80000000]
ACCEPTED_CUBES = [(4, 1), (4, 3), (8, 4), (12, 4), (2048, 12), (8192, 14)]
REFUSED_CUBES = [(0, 1), (6, 1), (8196, 1), (8, 5), (4, 0)]
FACES = {"ok": [4096, 8192, 16, 32, 48, 1 << 40], "null face pointer": [4096, 8192, 16, 0, 48, 64],
         "face blocks not 16-byte aligned": [4096, 8192, 16, 32, 48, 64 + 8]}


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """the program's answer to every description: {description line: [answer line, table lines ...]}"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler builds the oracle and the host library: it must be there"
    tmp = tmp_path_factory.mktemp("tex_chain")
    exe = tmp / "tex_chain_hostcheck"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                    "-o", str(exe), os.path.join(ROOT, "tools", "tex_chain_hostcheck.cpp")], check=True)
    lines = []
    for w, h, m in ACCEPTED_2D + [c[:3] for c in REFUSED_2D]:
        lines += [f"2d {w} {h} {m} {f | flag}" for f in STORED for flag in (0, BC1)]
    lines += [f"2d 8 8 2 {f}" for f in BAD_FORMATS]
    lines += [f"cube {s} {m}" for s, m in ACCEPTED_CUBES + REFUSED_CUBES]
    lines += ["faces " + " ".join(str(a) for a in addr) for addr in FACES.values()]
    (tmp / "list.txt").write_text("\n".join(lines) + "\n")
    run = subprocess.run([str(exe), str(tmp / "list.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-2000:]                # the sanitizers report nothing
    out, key = {}, None
    for text in run.stdout.splitlines():
        if text.startswith("  "):
            out[key].append(text.split()[1:])
        else:
            key = next(l for l in lines if text.startswith(l + " ") and l not in out)
            out[key] = [text[len(key) + 1:]]
    assert list(out) == lines
    return out


def test_2d_chains(answers):
    """every accepted shape in every stored format, as texels and as BC1 blocks: the byte count is structs.texture2d_bytes and
    bc1_ref.chain_bytes; first_block[l] is bc1_ref.level_offset / 8 up to [levels] = the chain's blocks and stays there to the table's
    end; first_texel[l] is the texel count of the l levels in front (structs.texture2d_bytes of the R8 chain); texel size, red / blue
    swap and alignment are the format's; a format with PBR_TEX_BC1_BLOCKS passes the table's check and not the stored-format one; and
    the level search gives l - 1 at first_block[l] - 1 and l at first_block[l]"""
    for w, h, m in ACCEPTED_2D:
        for f in STORED:
            for flag in (0, BC1):
                head, first_block, first_texel, search = answers[f"2d {w} {h} {m} {f | flag}"]
                nbytes = structs.texture2d_bytes(w, h, m, f | flag)
                assert nbytes == bc1_ref.chain_bytes(w, h, m, f | flag) > 0
                texel = bc1_ref.STORED[f]
                assert head == (f"bytes {nbytes} align {8 if flag else texel} stored {'unknown texture format' if flag else 'ok'} "
                                f"texel_bytes {texel} bgra {int(f in (structs.TEX_B8G8R8A8_UNORM, structs.TEX_B8G8R8A8_UNORM_SRGB))}"), (w, h, m, f, flag)
                want_blocks = [bc1_ref.level_offset(w, h, min(l, m)) // 8 for l in range(16)]
                assert [int(v) for v in first_block] == want_blocks, (w, h, m)
                assert 8 * want_blocks[m] == structs.texture2d_bytes(w, h, m, f | BC1)
                want_texels = [structs.texture2d_bytes(w, h, min(l, m), structs.TEX_R8_UNORM) if l else 0 for l in range(15)]
                assert [int(v) for v in first_texel] == want_texels, (w, h, m)
                assert [int(v) for v in search] == [v for l in range(1, m) for v in (l - 1, l)], (w, h, m)


def test_2d_refusals(answers):
    """a zero size, one above PBR_TEX_MAX_SIZE, too many levels or none, an unknown format, a stray bit beside the format: refused with
    the matching reason, and the byte count is 0, as in structs and bc1_ref"""
    for w, h, m, why in REFUSED_2D:
        for f in STORED:
            for flag in (0, BC1):
                (head,) = answers[f"2d {w} {h} {m} {f | flag}"]
                assert head.startswith("refused: ") and why in head, (w, h, m, head)
                assert structs.texture2d_bytes(w, h, m, f | flag) == bc1_ref.chain_bytes(w, h, m, f | flag) == 0
    for f in BAD_FORMATS:
        (head,) = answers[f"2d 8 8 2 {f}"]
        assert head == "refused: unknown texture format", (f, head)
        assert structs.texture2d_bytes(8, 8, 2, f) == bc1_ref.chain_bytes(8, 8, 2, f) == 0


def test_cube_chains(answers):
    """every accepted cube: the byte count is structs.bc6h_chain_bytes and bc6h_ref.chain_bytes; face_first[l] is the blocks of one face
    in front of level l, [levels] one face's blocks, constant from there; first_texel[l] is structs.cube_mip_offset; lanes is six faces'
    blocks; and the kernels' level search gives l - 1 and l either side of a level's first lane"""
    for s, m in ACCEPTED_CUBES:
        head, face_first, first_texel, search = answers[f"cube {s} {m}"]
        nbytes = structs.bc6h_chain_bytes(s, m)
        assert nbytes == bc6h_ref.chain_bytes(s, m) > 0
        want_first = [bc6h_ref.chain_bytes(s, min(l, m)) // 16 if l else 0 for l in range(15)]
        assert head == f"bytes {nbytes} lanes {6 * want_first[m]}", (s, m, head)
        assert [int(v) for v in face_first] == want_first and 16 * want_first[m] == nbytes, (s, m)
        assert [int(v) for v in first_texel] == [structs.cube_mip_offset(s, min(l, m)) for l in range(14)], (s, m)
        assert [int(v) for v in search] == [v for l in range(1, m) for v in (l - 1, l)], (s, m)


def test_cube_refusals_and_faces(answers):
    """size 0, no multiple of 4, above PBR_BC6H_MAX_SIZE, too many levels or none: refused, 0 bytes; a null or misaligned face pointer
    among the six is named"""
    for s, m in REFUSED_CUBES:
        (head,) = answers[f"cube {s} {m}"]
        assert head.startswith("refused: "), (s, m, head)
        assert structs.bc6h_chain_bytes(s, m) == bc6h_ref.chain_bytes(s, m) == 0
    for why, addr in FACES.items():
        (head,) = answers["faces " + " ".join(str(a) for a in addr)]
        assert head == ("ok" if why == "ok" else "refused: " + why)
