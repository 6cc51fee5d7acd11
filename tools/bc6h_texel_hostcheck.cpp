// bc6h_texel_hostcheck — csrc/bc6h_decode_block.hpp, the per-texel BC6H_UF16 decode the in-place sky resolve runs (k_skybox_bc6h), compiled
// for the host with its own main: built with -fsanitize=address,undefined by tests/test_sky_bc6h_cpu.py and held to the numpy
// restatement (tests/bc6h_ref.py) bit for bit.  Never loaded into Python, never run on a GPU.
//   bc6h_texel_hostcheck IN OUT
//   IN:  uint32 size, uint32 mips, then the six face chains (pbr_bc6h_chain_bytes(size, mips) bytes each, order px .. nz)
//   OUT: the pbr_cube_f32 layout as uint32 bit patterns: every texel of every level through header() + texel() + half_to_f32_bits(),
//        alpha 1.0f
// Every face lives in a heap buffer of exactly its chain's bytes, so a read past a chain is an ASan report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../direct12pbrrenderer_amd/csrc/bc6h_decode_block.hpp"

static uint32_t level_blocks(uint32_t s) { const uint32_t b = (s + 3u) / 4u; return b ? b : 1u; }

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t head[2];
    if (std::fread(head, 4, 2, in) != 2) { std::fprintf(stderr, "short header\n"); return 2; }
    const uint32_t size = head[0], mips = head[1];
    if (size < 4u || size > 8192u || (size & 3u) || mips < 1u || (size >> (mips - 1u)) < 1u) { std::fprintf(stderr, "bad cube\n"); return 2; }
    size_t chain = 0;
    for (uint32_t l = 0; l < mips; l++) chain += (size_t)16 * level_blocks(size >> l) * level_blocks(size >> l);
    uint8_t* face[6];
    for (int f = 0; f < 6; f++) {
        face[f] = (uint8_t*)std::malloc(chain);
        if (!face[f] || std::fread(face[f], 1, chain, in) != chain) { std::fprintf(stderr, "short face %d\n", f); return 2; }
    }
    std::fclose(in);

    std::vector<uint32_t> out;
    size_t first = 0;                                     // bytes of a face in front of the level
    for (uint32_t l = 0; l < mips; l++) {
        const uint32_t s = size >> l, bw = level_blocks(s);
        for (int f = 0; f < 6; f++)
            for (uint32_t y = 0; y < s; y++)
                for (uint32_t x = 0; x < s; x++) {
                    uint32_t q[4];
                    std::memcpy(q, face[f] + first + (size_t)16 * ((y >> 2) * bw + (x >> 2)), 16);
                    const bc6h_dec::Block b = bc6h_dec::header(q[0], q[1], q[2], q[3]);     // (per texel here: the check is of values, not of cost)
                    uint32_t half[3];
                    bc6h_dec::texel(b, 4u * (y & 3u) + (x & 3u), half);
                    for (int c = 0; c < 3; c++) out.push_back(bc6h_dec::half_to_f32_bits(half[c]));
                    out.push_back(0x3f800000u);
                }
        first += (size_t)16 * bw * bw;
    }
    for (int f = 0; f < 6; f++) std::free(face[f]);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o || std::fwrite(out.data(), 4, out.size(), o) != out.size()) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    std::fclose(o);
    return 0;
}
