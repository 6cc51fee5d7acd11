// tex_chain_hostcheck — csrc/tex_chain.hpp, the chain geometry every texture entry point shares, compiled for the host with its own
// main: built with -fsanitize=address,undefined by tests/test_tex_chain_cpu.py and held to the Python restatements (structs.py,
// tests/bc1_ref.py, tests/bc6h_ref.py).  Never loaded into Python, never run on a GPU.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -Wextra -o tex_chain_hostcheck tools/tex_chain_hostcheck.cpp
//   tex_chain_hostcheck LIST
// LIST holds one description per line; the answer to each goes to stdout, in the same order:
//   2d W H MIPS FORMAT     (FORMAT: a PBR_TEX_* number, with or without PBR_TEX_BC1_BLOCKS, or anything else)
//       2d W H MIPS FORMAT refused: WHY
//       2d W H MIPS FORMAT bytes N align A stored STORED_WHY|ok texel_bytes T bgra B
//         first_block  the sixteen entries          first_texel  the fifteen entries
//         search       level_of_block at first_block[l] - 1 and at first_block[l], for l = 1 .. MIPS - 1
//     `refused` is the check of pbr_texture2d_bytes and pbr_gbuffer_raster with maps (the flag allowed), `stored` that of
//     pbr_texture2d_gen_mips, pbr_bc1_encode and pbr_bc1_decode (a stored format alone); A is the alignment tex2d::aligned asks for.
//   cube SIZE MIPS
//       cube SIZE MIPS refused: WHY
//       cube SIZE MIPS bytes N lanes L
//         face_first   the fifteen entries          first_texel  the fourteen entries
//         search       the level the cube kernels' unrolled search gives lane 6 face_first[l] - 1 and lane 6 face_first[l]
//   faces A0 A1 A2 A3 A4 A5   (six addresses, never dereferenced)
//       faces A0 A1 A2 A3 A4 A5 ok | refused: WHY
#include <cstdio>
#include <cstring>

#include "../direct12pbrrenderer_amd/csrc/tex_chain.hpp"

// the search k_bc6h_decode_cube and bc6h_enc::encode_lane run on the table (theirs is unrolled over static indices)
static uint32_t cube_level_of_lane(const bc6h_chain::Cube<const void*>& L, uint32_t g) {
    uint32_t l = 0;
    for (uint32_t k = 1; k < bc6h_chain::MAX_LEVELS; k++)
        if (k < L.mips && g >= 6u * L.face_first[k]) l = k;
    return l;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s LIST\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "r");
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char line[256];
    while (std::fgets(line, sizeof line, in)) {
        unsigned w, h, m, f;
        unsigned long long a[6];
        if (std::sscanf(line, "2d %u %u %u %u", &w, &h, &m, &f) == 4) {
            std::printf("2d %u %u %u %u ", w, h, m, f);
            if (const char* why = tex2d::refusal(w, h, m, f, true)) {
                if (tex2d::chain_bytes(w, h, m, f) != 0) { std::fprintf(stderr, "a refused chain has bytes\n"); return 1; }
                std::printf("refused: %s\n", why);
                continue;
            }
            uintptr_t align = 1;
            while (!tex2d::aligned((const void*)align, f)) align <<= 1;
            const char* stored = tex2d::refusal(w, h, m, f);
            tex2d::Levels L;
            std::memset(&L, 0xa5, sizeof L);
            tex2d::fill(L, w, h, m, f & 0xffu);
            std::printf("bytes %zu align %zu stored %s texel_bytes %u bgra %u\n", tex2d::chain_bytes(w, h, m, f), (size_t)align,
                        stored ? stored : "ok", L.texel_bytes, L.bgra);
            if (L.width != w || L.height != h || L.mips != m) { std::fprintf(stderr, "the table's description\n"); return 1; }
            std::printf("  first_block");
            for (uint32_t l = 0; l <= tex2d::MAX_LEVELS; l++) std::printf(" %u", L.first_block[l]);
            std::printf("\n  first_texel");
            for (uint32_t l = 0; l < tex2d::MAX_LEVELS; l++) std::printf(" %llu", (unsigned long long)L.first_texel[l]);
            std::printf("\n  search");
            for (uint32_t l = 1; l < m; l++)
                std::printf(" %u %u", tex2d::level_of_block(L, L.first_block[l] - 1u), tex2d::level_of_block(L, L.first_block[l]));
            std::printf("\n");
        } else if (std::sscanf(line, "cube %u %u", &w, &m) == 2) {
            std::printf("cube %u %u ", w, m);
            if (const char* why = bc6h_chain::refusal(w, m)) {
                if (bc6h_chain::chain_ok(w, m) || bc6h_chain::chain_bytes(w, m) != 0) { std::fprintf(stderr, "a refused cube is ok\n"); return 1; }
                std::printf("refused: %s\n", why);
                continue;
            }
            bc6h_chain::Cube<const void*> L;
            std::memset(&L, 0xa5, sizeof L);
            bc6h_chain::fill(L, w, m);
            if (!bc6h_chain::chain_ok(w, m) || L.size != w || L.mips != m) { std::fprintf(stderr, "the table's description\n"); return 1; }
            std::printf("bytes %zu lanes %u\n  face_first", bc6h_chain::chain_bytes(w, m), L.lanes);
            for (uint32_t l = 0; l <= bc6h_chain::MAX_LEVELS; l++) std::printf(" %u", L.face_first[l]);
            std::printf("\n  first_texel");
            for (uint32_t l = 0; l < bc6h_chain::MAX_LEVELS; l++) std::printf(" %u", L.first_texel[l]);
            std::printf("\n  search");
            for (uint32_t l = 1; l < m; l++)
                std::printf(" %u %u", cube_level_of_lane(L, 6u * L.face_first[l] - 1u), cube_level_of_lane(L, 6u * L.face_first[l]));
            std::printf("\n");
        } else if (std::sscanf(line, "faces %llu %llu %llu %llu %llu %llu", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) == 6) {
            const void* face[6];
            for (int i = 0; i < 6; i++) face[i] = (const void*)(uintptr_t)a[i];
            std::printf("faces %llu %llu %llu %llu %llu %llu ", a[0], a[1], a[2], a[3], a[4], a[5]);
            if (const char* why = bc6h_chain::faces_refusal(face)) std::printf("refused: %s\n", why);
            else std::printf("ok\n");
        } else {
            std::fprintf(stderr, "bad line: %s", line);
            return 2;
        }
    }
    std::fclose(in);
    return 0;
}
