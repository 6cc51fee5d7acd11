// bc6h_encode_hostcheck.cpp — the body of k_bc6h_encode_cube (csrc/bc6h_encode_block.hpp) compiled for the host, lane after lane, in a
// program of its own: built with -fsanitize=address,undefined and compared with tests/bc6h_encode_ref.py by tests/test_bc6h_encode_cpu.py
// (and by hand: tools/README.md).  Input file: uint32 size, uint32 mip_levels, the pbr_cube_f32 chain as fp32 RGBA.  Output file: the
// six face chains one after the other.  A third argument `two_region` runs the lane of k_bc6h_encode_cube2 (PBR_BC6H_ENCODE_TWO_REGION,
// compared with tests/bc6h_encode2_ref.py by tests/test_bc6h_encode2_cpu.py).  Every buffer is exactly as large as the entry point's contract says, so an access outside it
// is an ASan report.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o bc6h_encode_hostcheck tools/bc6h_encode_hostcheck.cpp
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../direct12pbrrenderer_amd/csrc/bc6h_encode_block.hpp"

int main(int argc, char** argv) {
    const bool two = argc == 4 && std::strcmp(argv[3], "two_region") == 0;
    if (argc != 3 && !two) { std::fprintf(stderr, "usage: %s cube.bin blocks.bin [two_region]\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t head[2];
    if (std::fread(head, 4, 2, in) != 2) { std::fprintf(stderr, "truncated header\n"); return 2; }
    const uint32_t size = head[0], mips = head[1];
    if (!bc6h_chain::chain_ok(size, mips)) { std::fprintf(stderr, "bad cube description\n"); return 2; }
    bc6h_enc::Cube L;
    bc6h_chain::fill(L, size, mips);
    const size_t texels = (size_t)L.first_texel[mips - 1] + 6u * (size_t)(size >> (mips - 1)) * (size >> (mips - 1));
    std::vector<bc6h_enc::Texel> cube(texels);
    if (std::fread(cube.data(), 16, texels, in) != texels) { std::fprintf(stderr, "truncated cube\n"); return 2; }
    std::fclose(in);
    const size_t face_blocks = L.face_first[mips];
    std::vector<bc6h_enc::Block> faces[6];
    for (int f = 0; f < 6; f++) {
        faces[f].assign(face_blocks, bc6h_enc::Block{0x5a5a5a5au, 0x5a5a5a5au, 0x5a5a5a5au, 0x5a5a5a5au});
        L.face[f] = faces[f].data();
    }
    for (uint32_t g = 0; g < L.lanes; g++) {
        if (two) bc6h_enc::encode_lane<true>(L, g, cube.data());
        else bc6h_enc::encode_lane(L, g, cube.data());
    }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    for (int f = 0; f < 6; f++)
        if (std::fwrite(faces[f].data(), 16, face_blocks, out) != face_blocks) return 2;
    std::fclose(out);
    return 0;
}
