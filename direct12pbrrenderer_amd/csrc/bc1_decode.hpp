// bc1_decode.hpp — the BC1 block decode pinned in include/pbr_hip.h (PBR_TEX_BC1_BLOCKS), shared by the textured raster's sampler
// (BC1-resident textures, read in place: tex_sampler.hpp) and, in texture2d.hip, the bulk decoder (pbr_bc1_decode) and the encoder's
// fit (pbr_bc1_encode).  The block decode only: where a block lies in a chain is tex_chain.hpp's.
// A block is 8 bytes, read as two little-endian words: `endpoints` = c0 | c1 << 16 (RGB565 each) and `bits` = 16 2-bit palette
// indices, texel (x, y) of the block at bit 2 (4 y + x).  A palette entry is R | G << 8 | B << 16 | A << 24 whatever the stored
// format: the callers swizzle (the sampler when it picks channels, the bulk decoder when it stores).
// tests/bc1_ref.py restates the rule in numpy, independently of this file.
#pragma once

// an RGB565 endpoint's channels expanded to 8 bits by bit replication
__device__ __forceinline__ void bc1_expand565(uint32_t c, uint32_t& r, uint32_t& g, uint32_t& b) {
    const uint32_t r5 = (c >> 11) & 31u, g6 = (c >> 5) & 63u, b5 = c & 31u;
    r = (r5 << 3) | (r5 >> 2);
    g = (g6 << 2) | (g6 >> 4);
    b = (b5 << 3) | (b5 >> 2);
}

// the block's four colours.  c0 > c1: the two thirds, opaque; else the midpoint and transparent black
__device__ __forceinline__ void bc1_palette(uint32_t endpoints, uint32_t pal[4]) {
    const uint32_t c0 = endpoints & 0xffffu, c1 = endpoints >> 16;
    uint32_t r0, g0, b0, r1, g1, b1;
    bc1_expand565(c0, r0, g0, b0);
    bc1_expand565(c1, r1, g1, b1);
    const bool four = c0 > c1;
    const uint32_t r2 = four ? (2u * r0 + r1 + 1u) / 3u : (r0 + r1 + 1u) >> 1, r3 = four ? (r0 + 2u * r1 + 1u) / 3u : 0u;
    const uint32_t g2 = four ? (2u * g0 + g1 + 1u) / 3u : (g0 + g1 + 1u) >> 1, g3 = four ? (g0 + 2u * g1 + 1u) / 3u : 0u;
    const uint32_t b2 = four ? (2u * b0 + b1 + 1u) / 3u : (b0 + b1 + 1u) >> 1, b3 = four ? (b0 + 2u * b1 + 1u) / 3u : 0u;
    pal[0] = r0 | (g0 << 8) | (b0 << 16) | 0xff000000u;
    pal[1] = r1 | (g1 << 8) | (b1 << 16) | 0xff000000u;
    pal[2] = r2 | (g2 << 8) | (b2 << 16) | 0xff000000u;
    pal[3] = r3 | (g3 << 8) | (b3 << 16) | (four ? 0xff000000u : 0u);
}

// texel (x, y) of the block, x, y in [0, 4): its palette entry, by selects (no indexed register array)
__device__ __forceinline__ uint32_t bc1_texel(const uint32_t pal[4], uint32_t bits, uint32_t x, uint32_t y) {
    const uint32_t k = bits >> (2u * (4u * y + x));
    const uint32_t lo = (k & 1u) ? pal[1] : pal[0], hi = (k & 1u) ? pal[3] : pal[2];
    return (k & 2u) ? hi : lo;
}

// a palette entry as one texel of the stored format (the 4-byte ones: R8G8B8A8 as it is, B8G8R8A8[_SRGB] with red and blue swapped)
__device__ __forceinline__ uint32_t bc1_stored(uint32_t rgba, bool bgra) {
    return bgra ? (rgba & 0xff00ff00u) | ((rgba >> 16) & 0xffu) | ((rgba & 0xffu) << 16) : rgba;
}
