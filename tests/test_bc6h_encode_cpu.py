"""The BC6H_UF16 encoding rule on the CPU (include/pbr_hip.h: pbr_bc6h_encode_cube): the numpy restatement tests/bc6h_encode_ref.py
against the decoder it did not write (bc6h_ref.decode_blocks, itself held to a third-party decoder in tests/test_bc6h_cpu.py), its
quality against the test-side yardstick bc6h_ref.encode_mode3, the pinned special values, the cube-map file around its chains, and
the kernel's own text (csrc/bc6h_encode_block.hpp) compiled for the host in a stand-alone program under ASan / UBSan against the
restatement.  No GPU; reads tests/golden/ only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bc6h_encode_ref as enc
import bc6h_ref
from direct12pbrrenderer_amd import host, synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def smooth():
    """level 0 of the fixture's analytic sky (gradient + a sun lobe of about 50), float32 [6, 32, 32, 3]"""
    return dict(np.load(os.path.join(HERE, "golden", "sky_bc6h.npz"), allow_pickle=False))["smooth_level0"]


def noisy_level0():
    return synth.env_cube(32, 1, 7).reshape(6, 32, 32, 4)[..., :3]


def random_level0():
    return (np.random.default_rng(16).random((6, 16, 16, 3)) ** 4 * 200).astype(np.float32)


def inputs(smooth):
    """name -> the levels of a cube, each float32 [6, s, s, 3]: the fp32 2 x 2 box chain of its level 0"""
    return {
        "smooth 32^2": enc.box_mips(smooth, 6),
        "noisy 32^2": enc.box_mips(noisy_level0(), 6),
        "random 16^2": enc.box_mips(random_level0(), 5),
        "smooth crop 12^2": enc.box_mips(smooth[:, :12, :12], 4),
    }


def decoded_error(blocks, h, inside):
    """squared error in half-code space of the blocks as bc6h_ref decodes them, per block, over the texels inside the level"""
    return np.where(inside[..., None], (bc6h_ref.decode_blocks(blocks) - h) ** 2, 0).sum(axis=(1, 2))


def level_errors(img):
    """one face level -> per block (the encoder's predicted error, its decoded error, the yardstick's decoded error, modes, blocks)"""
    h, inside = enc.level_texels(img)
    blocks, predicted, mode = enc.encode_level(img)
    return predicted, decoded_error(blocks, h, inside), decoded_error(bc6h_ref.encode_mode3(img), h, inside), mode, blocks


def test_restatement_against_the_decoder_it_did_not_write(smooth):
    """every block of every input, decoded by bc6h_ref.decode_blocks, has exactly the error the encoder predicted for it; only the four
    one-region modes occur, and every anchor index is below 8: encode_blocks asserts it before it stores the index's three low bits, and
    a dropped high bit would show as a decoded error that differs from the predicted one"""
    sizes = {"smooth 32^2": [32, 16, 8, 4, 2, 1], "noisy 32^2": [32, 16, 8, 4, 2, 1], "random 16^2": [16, 8, 4, 2, 1], "smooth crop 12^2": [12, 6, 3, 1]}
    for name, levels in inputs(smooth).items():
        assert [l.shape[1] for l in levels] == sizes[name]
        n = 0
        for img in levels:
            for f in range(6):
                predicted, got, _, mode, blocks = level_errors(img[f])
                assert np.array_equal(predicted, got), (name, img.shape, f)
                assert np.isin(mode, (0x03, 0x07, 0x0B, 0x0F)).all() and np.array_equal(mode, bc6h_ref.block_modes(blocks))
                assert bc6h_ref.decode_blocks(blocks).max() <= 0x7BFF
                n += len(blocks)
        assert n == {"smooth 32^2": 522, "noisy 32^2": 522, "random 16^2": 138, "smooth crop 12^2": 90}[name]


def test_quality_against_the_yardstick_on_the_smooth_fixture(smooth):
    """On each of the six levels of the fixture sky, summed over the faces, the squared error is at most that of bc6h_ref.encode_mode3,
    and no block is worse than the yardstick's.  A condition, not a tolerance; the ratios measured (printed below, and in
    profiles/bc6h_encode_ms.txt and DESIGN.md): 0.547, 0.421, 0.777, 0.640, 0.642 and 0 (the 1 x 1 level is exact)."""
    ratios = []
    for img in enc.box_mips(smooth, 6):
        ours = theirs = 0
        for f in range(6):
            _, got, yard, _, _ = level_errors(img[f])
            assert (got <= yard).all(), (img.shape, f, int((got > yard).sum()))
            ours, theirs = ours + int(got.sum()), theirs + int(yard.sum())
        assert ours <= theirs
        ratios.append(ours / theirs)
    print("bc6h encode, smooth fixture, encoder error / yardstick error per level:", ", ".join(f"{r:.3f}" for r in ratios))
    assert ratios[-1] == 0.0


def test_noisy_and_random_inputs_against_the_yardstick(smooth):
    """the noisy analytic sky, seeded heavy-tailed noise and the 12^2 crop (partial blocks on levels of 6 and 3), whole chains: the summed
    error is at most the yardstick's and at most 2 % of the blocks are worse than the yardstick's.  Measured: 0.545 with 1 block of 522
    worse, 0.736 with 2 of 138, 0.437 with none of 90."""
    for name, levels in inputs(smooth).items():
        if name == "smooth 32^2":
            continue
        ours = theirs = worse = n = 0
        for img in levels:
            for f in range(6):
                _, got, yard, _, _ = level_errors(img[f])
                ours, theirs, worse, n = ours + int(got.sum()), theirs + int(yard.sum()), worse + int((got > yard).sum()), n + len(got)
        print(f"bc6h encode, {name}: encoder error / yardstick error {ours / theirs:.3f}, {worse} of {n} blocks worse")
        assert ours <= theirs and worse <= 0.02 * n, (name, ours, theirs, worse, n)


def test_special_values_take_the_pinned_codes():
    """NaN, +-inf, negatives, -0.0, 1e9, 65504, the values around the half grid (round up, round down, exact ties to even), subnormal
    halves and what underflows: each gives the pinned code; a block of each decodes to that code (<= 0x7BFF) exactly, through mode 0x0f"""
    cases = [
        (np.nan, 0), (-np.nan, 0), (np.inf, 0x7BFF), (-np.inf, 0), (-1.0, 0), (-1e-30, 0), (-0.0, 0), (0.0, 0), (1e9, 0x7BFF),
        (65504.0, 0x7BFF), (65519.9, 0x7BFF), (65520.0, 0x7BFF), (65503.0, 0x7BFF), (65488.0, 0x7BFE),       # 65488 is the tie below 65504: to even
        (1.0, 0x3C00), (1.0 + 2.0 ** -11, 0x3C00), (1.0 + 2.0 ** -11 + 2.0 ** -20, 0x3C01), (1.0 + 3 * 2.0 ** -11, 0x3C02),
        (1.0 + 2.0 ** -10, 0x3C01), (2.0 - 2.0 ** -12, 0x4000),                                               # rounds up into the next exponent
        (6e-8, 1), (3e-5, 503), (2.0 ** -24, 1), (2.0 ** -25, 0), (2.0 ** -25 * 1.0001, 1), (1.5 * 2.0 ** -24, 2), (2.5 * 2.0 ** -24, 2),
        (2.0 ** -14, 0x0400), (2.0 ** -14 - 2.0 ** -26, 0x0400), (1e-40, 0), (1e-9, 0),
    ]
    values = np.float32([v for v, _ in cases])
    want = np.int64([c for _, c in cases])
    assert round(3e-5 * 2 ** 24) == 503
    assert np.array_equal(enc.half_code(values), want)
    assert np.signbit(np.float32(-0.0)) and enc.half_code(np.float32(-0.0)) == 0          # not 0x8000
    for v, c in zip(values, want):
        img = np.full((4, 4, 3), v, np.float32)
        blocks, predicted, mode = enc.encode_level(img)
        assert mode[0] == 0x0F and predicted[0] == 0
        assert (bc6h_ref.decode_blocks(blocks) == c).all() and c <= 0x7BFF, (v, c)
    # all of them scattered over one level, specials next to ordinary texels
    rng = np.random.default_rng(3)
    img = (rng.random((8, 8, 3)) * 4).astype(np.float32)
    img.reshape(-1)[rng.permutation(img.size)[:len(values)]] = values
    h, inside = enc.level_texels(img)
    blocks, predicted, _ = enc.encode_level(img)
    assert np.array_equal(decoded_error(blocks, h, inside), predicted) and bc6h_ref.decode_blocks(blocks).max() <= 0x7BFF


def test_constant_blocks_are_exact(smooth):
    """a block of one colour, partial blocks included, takes mode 0x0f and decodes to its half codes exactly"""
    rng = np.random.default_rng(4)
    for s in (1, 2, 3, 4):
        for _ in range(8):
            colour = (rng.random(3) ** 6 * 65000).astype(np.float32)
            img = np.broadcast_to(colour, (s, s, 3))
            blocks, predicted, mode = enc.encode_level(img)
            assert mode[0] == 0x0F and predicted[0] == 0
            dec = bc6h_ref.decode_blocks(blocks)[0].reshape(4, 4, 3)[:s, :s]
            assert (dec == enc.half_code(colour)).all()


def test_file_round_trip_of_encoded_chains(smooth):
    """host.write_cubemap_file of the encoded chains, then parse_cubemap_file: the same bytes at the reported offsets, the same pack"""
    levels = enc.box_mips(smooth, 6)
    cube = np.concatenate([np.concatenate([l, np.ones(l.shape[:3] + (1,), np.float32)], axis=-1).reshape(-1, 4) for l in levels])
    faces = enc.encode_cube(cube, 32, 6)
    assert all(f.size == bc6h_ref.chain_bytes(32, 6) for f in faces)
    sh = np.random.default_rng(5).standard_normal(28).astype(np.float32)
    data = host.write_cubemap_file(faces, 32, 6, sh)
    size, mips, offsets, got_sh = host.parse_cubemap_file(data)
    assert (size, mips) == (32, 6) and np.array_equal(got_sh.view(np.uint32), sh.view(np.uint32))
    for f, o in enumerate(offsets):
        assert data[o:o + faces[f].size] == faces[f].tobytes()
    # and what the file decodes to is what the encoder predicted, through the decode restatement's own chain walk
    dec = bc6h_ref.decode_cube([np.frombuffer(data, np.uint8)[o:o + faces[0].size] for o in offsets], size, mips)
    total = sum(int(level_errors(img[f])[0].sum()) for img in levels for f in range(6))
    assert int(((enc.half_code(dec[:, :3]) - enc.half_code(cube[:, :3])) ** 2).sum()) == total


def test_host_entry_points_are_exported():
    lib = host.load()
    assert lib.pbrh_import_cubemap and lib.pbrh_import_cubemap_dir
    from direct12pbrrenderer_amd import _lib
    assert _lib.load().pbr_bc6h_encode_cube


def test_kernel_text_on_the_host_under_sanitizers(smooth, tmp_path):
    """csrc/bc6h_encode_block.hpp — the text k_bc6h_encode_cube runs, from the lane's number to the stored block — compiled for the host
    with -fsanitize=address,undefined in a program of its own (tools/bc6h_encode_hostcheck.cpp; every buffer exactly as large as the
    entry point's contract) equals the restatement byte for byte on the 4^2 x 3, 12^2 x 4 and 32^2 x 6 cubes, specials scattered in"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler builds the oracle and the host library: it must be there"
    exe = tmp_path / "bc6h_encode_hostcheck"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                    "-o", str(exe), os.path.join(ROOT, "tools", "bc6h_encode_hostcheck.cpp")], check=True)
    rng = np.random.default_rng(6)
    specials = np.float32([np.nan, np.inf, -np.inf, -1.0, -0.0, 1e9, 65504.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 6e-8, 3e-5, 2.0 ** -25])
    cubes = {(4, 3): (rng.random((6, 4, 4, 3)) ** 4 * 200).astype(np.float32), (12, 4): smooth[:, :12, :12], (32, 6): smooth.copy()}
    cubes[(32, 6)][2].reshape(-1)[rng.permutation(32 * 32 * 3)[:len(specials)]] = specials
    cubes[(4, 3)][1].reshape(-1)[:len(specials)] = specials
    for (size, mips), level0 in cubes.items():
        with np.errstate(invalid="ignore", over="ignore"):
            levels = enc.box_mips(level0, mips)
        cube = np.concatenate([np.concatenate([l, np.ones(l.shape[:3] + (1,), np.float32)], axis=-1).reshape(-1, 4) for l in levels])
        (tmp_path / "cube.bin").write_bytes(np.uint32([size, mips]).tobytes() + cube.astype(np.float32).tobytes())
        run = subprocess.run([str(exe), str(tmp_path / "cube.bin"), str(tmp_path / "blocks.bin")], capture_output=True, text=True)
        assert run.returncode == 0 and not run.stderr, run.stderr[-2000:]
        n = bc6h_ref.chain_bytes(size, mips)
        got = np.fromfile(tmp_path / "blocks.bin", np.uint8).reshape(6, n)
        want = enc.encode_cube(cube, size, mips)
        for f in range(6):
            assert np.array_equal(got[f], want[f]), (size, mips, f)
