// fxaa_hostcheck.cpp — the per-pixel rule of k_fxaa (csrc/fxaa_pixel.hpp) compiled for the host, pixel after pixel, in a program of its
// own: built with -fsanitize=address,undefined and compared with tests/fxaa_ref.py by tests/test_fxaa_cpu.py (and by hand:
// tools/README.md).  Input file: uint32 w, h, pitch, then h x pitch RGBA8 pixels.  Output file: h x pitch pixels, the filtered image in
// the first w of every row and 0x5a5a5a5a in the rest.  Both buffers are exactly h x pitch pixels, so a read or write outside the image's
// memory is an ASan report.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o fxaa_hostcheck tools/fxaa_hostcheck.cpp
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../direct12pbrrenderer_amd/csrc/fxaa_pixel.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s image.bin filtered.bin\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t head[3];
    if (std::fread(head, 4, 3, in) != 3) { std::fprintf(stderr, "truncated header\n"); return 2; }
    const uint32_t w = head[0], h = head[1], pitch = head[2];
    if (!w || !h || pitch < w || w > 16384u || h > 16384u || pitch > 32768u) { std::fprintf(stderr, "bad image description\n"); return 2; }
    const size_t n = (size_t)h * pitch;
    std::vector<uint32_t> src(n), dst(n, 0x5a5a5a5au);
    if (std::fread(src.data(), 4, n, in) != n) { std::fprintf(stderr, "truncated image\n"); return 2; }
    std::fclose(in);
    const fxaa::MemoryFetch f{src.data(), pitch};
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) dst[(size_t)y * pitch + x] = fxaa::pixel(f, (int)x, (int)y, (int)w, (int)h);
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    if (std::fwrite(dst.data(), 4, n, out) != n) return 2;
    std::fclose(out);
    return 0;
}
