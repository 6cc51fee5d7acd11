// tex_chain.hpp — the geometry of the two block-compressed mip chains of include/pbr_hip.h, in one place: how many levels a chain may
// have, where a level's first texel or block lies, how many blocks a level holds, which descriptions are refused, and the level tables
// the chain kernels take as an argument.
//   tex2d       the chain of a pbr_texture2d, as texels of a stored format or as BC1 blocks (PBR_TEX_BC1_BLOCKS): texture2d.hip
//               (pbr_texture2d_gen_mips, pbr_bc1_encode, pbr_bc1_decode, pbr_texture2d_bytes) and the texture table of
//               pbr_gbuffer_raster with maps (gbuffer_raster.hip)
//   bc6h_chain  the six BC6H_UF16 face chains of a sky cube beside the pbr_cube_f32 chain: bc6h_decode.hip, bc6h_encode.hip
//               (bc6h_encode_block.hpp) and the resident sky (pbr_skybox_bc6h, raster.hip)
// Plain C++: hipcc compiles it for gfx950, tools/tex_chain_hostcheck.cpp for the host, where it runs under ASan / UBSan against the
// Python restatements (structs.py, tests/bc1_ref.py, tests/bc6h_ref.py).  A table struct keeps the field order its kernels have always
// taken, so no kernel argument moves.
#pragma once
#include <cstdint>
#include <cstddef>
#include "../../include/pbr_hip.h"

#if defined(__HIPCC__)
#define TEX_CHAIN_FN __host__ __device__ inline      // called by kernels too
#else
#define TEX_CHAIN_FN inline
#endif

namespace tex2d {

constexpr uint32_t MAX_LEVELS = 15;        // floor(log2(PBR_TEX_MAX_SIZE)) + 1
static_assert((1u << (MAX_LEVELS - 1)) == PBR_TEX_MAX_SIZE, "levels of the largest chain");

// floor(log2(min(w, h))) + 1: the levels of a full chain down to a 1-texel side
inline uint32_t max_mip_levels(uint32_t w, uint32_t h) {
    uint32_t m = w < h ? w : h, n = 0;
    while (m) { n++; m >>= 1; }
    return n;
}
inline bool stored_format(uint32_t f) {
    return f == PBR_TEX_R8_UNORM || f == PBR_TEX_R8G8B8A8_UNORM || f == PBR_TEX_B8G8R8A8_UNORM || f == PBR_TEX_B8G8R8A8_UNORM_SRGB;
}
inline uint32_t texel_bytes(uint32_t stored) { return stored == PBR_TEX_R8_UNORM ? 1u : 4u; }
// red and blue swapped in the stored texel
inline bool bgra(uint32_t stored) { return stored == PBR_TEX_B8G8R8A8_UNORM || stored == PBR_TEX_B8G8R8A8_UNORM_SRGB; }
// blocks across (or down) a level of n texels: at least one
TEX_CHAIN_FN uint32_t bc1_blocks(uint32_t n) { return n > 4u ? (n + 3u) >> 2 : 1u; }

// what is wrong with a chain's description; nullptr: nothing.  `format` is a stored format; `blocks_flag`: PBR_TEX_BC1_BLOCKS may be set in it
inline const char* refusal(uint32_t width, uint32_t height, uint32_t mip_levels, uint32_t format, bool blocks_flag = false) {
    if ((format & ~(0xffu | (blocks_flag ? PBR_TEX_BC1_BLOCKS : 0u))) != 0 || !stored_format(format & 0xffu)) return "unknown texture format";
    if (!width || !height || width > PBR_TEX_MAX_SIZE || height > PBR_TEX_MAX_SIZE) return "texture size zero or above PBR_TEX_MAX_SIZE";
    if (!mip_levels || mip_levels > max_mip_levels(width, height)) return "mip_levels 0 or above floor(log2(min(w, h))) + 1";
    return nullptr;
}
// the alignment of a chain's first byte: the texel size, 8 bytes for BC1 blocks
inline bool aligned(const void* p, uint32_t format) {
    const uintptr_t a = (format & PBR_TEX_BC1_BLOCKS) ? 8u : texel_bytes(format & 0xffu);
    return ((uintptr_t)p & (a - 1u)) == 0;
}

// the level table of a launch over a whole chain (k_bc1_decode, k_bc1_encode)
struct Levels {
    uint32_t first_block[MAX_LEVELS + 1];  // the level's first block in the chain; [mips] = the chain's blocks
    uint64_t first_texel[MAX_LEVELS];      // the level's first texel in the uncompressed chain
    uint32_t width, height, mips;
    uint32_t texel_bytes;                  // 4, or 1 (R8)
    uint32_t bgra;                         // B8G8R8A8[_SRGB]: red and blue swapped in the stored texel
};
// fills the table of a description refusal() accepts; returns the chain's texels
inline uint64_t fill(Levels& L, uint32_t width, uint32_t height, uint32_t mip_levels, uint32_t stored) {
    L.width = width; L.height = height; L.mips = mip_levels;
    L.texel_bytes = texel_bytes(stored);
    L.bgra = bgra(stored);
    uint64_t nb = 0, nt = 0;
    for (uint32_t l = 0; l <= MAX_LEVELS; l++) {
        L.first_block[l] = (uint32_t)nb;          // (the largest chain holds 4096^2 * 4 / 3 blocks: below 2^32)
        if (l < MAX_LEVELS) L.first_texel[l] = nt;
        if (l < mip_levels) {
            nb += (uint64_t)bc1_blocks(width >> l) * bc1_blocks(height >> l);
            nt += (uint64_t)(width >> l) * (height >> l);
        }
    }
    return nt;
}
// the level of block b < L.first_block[L.mips]
TEX_CHAIN_FN uint32_t level_of_block(const Levels& L, uint32_t b) {
    uint32_t l = 0;
    while (l + 1u < L.mips && b >= L.first_block[l + 1u]) l++;
    return l;
}
// pbr_texture2d_bytes: the bytes of a whole chain of either kind, 0 for a refused description
inline size_t chain_bytes(uint32_t width, uint32_t height, uint32_t mip_levels, uint32_t format) {
    if (refusal(width, height, mip_levels, format, true)) return 0;
    Levels L;
    const uint64_t texels = fill(L, width, height, mip_levels, format & 0xffu);
    return (format & PBR_TEX_BC1_BLOCKS) ? (size_t)L.first_block[mip_levels] * 8 : (size_t)texels * L.texel_bytes;
}

}  // namespace tex2d

namespace bc6h_chain {

constexpr uint32_t MAX_LEVELS = 14;        // floor(log2(PBR_BC6H_MAX_SIZE)) + 1
static_assert((1u << (MAX_LEVELS - 1)) == PBR_BC6H_MAX_SIZE, "levels of the largest cube");

inline uint32_t max_levels(uint32_t size) {
    uint32_t n = 0;
    while (size) { n++; size >>= 1; }
    return n;
}
// blocks across a level of s texels: at least one
inline uint32_t level_blocks(uint32_t s) { const uint32_t b = (s + 3u) / 4u; return b ? b : 1u; }
inline bool chain_ok(uint32_t size, uint32_t mip_levels) {
    return size >= 4u && size <= PBR_BC6H_MAX_SIZE && (size & 3u) == 0 && mip_levels >= 1u && mip_levels <= max_levels(size);
}
// what is wrong with a cube's description; nullptr: nothing
inline const char* refusal(uint32_t size, uint32_t mip_levels) {
    return chain_ok(size, mip_levels) ? nullptr
         : "size 0, not a multiple of 4 or above PBR_BC6H_MAX_SIZE, or mip_levels 0 or above floor(log2(size)) + 1";
}
// what is wrong with the six face pointers of a cube; nullptr: nothing
inline const char* faces_refusal(const void* const face[6]) {
    for (int f = 0; f < 6; f++) {
        if (!face[f]) return "null face pointer";
        if ((uintptr_t)face[f] & 15u) return "face blocks not 16-byte aligned";
    }
    return nullptr;
}

// the level table of a launch over a whole cube (k_bc6h_decode_cube, k_bc6h_encode_cube); Face: the pointer type its kernel reads
template <class Face>
struct Cube {
    Face face[6];
    uint32_t face_first[MAX_LEVELS + 1];   // blocks of one face in front of the level; [mips] = one face's blocks
    uint32_t first_texel[MAX_LEVELS];      // pbr_cube_mip_offset of the level
    uint32_t size, mips;
    uint32_t lanes;                        // 6 x one face's blocks
};
// fills everything but the faces, for a description chain_ok() accepts
template <class Face>
inline void fill(Cube<Face>& L, uint32_t size, uint32_t mip_levels) {
    L.size = size; L.mips = mip_levels;
    uint32_t nb = 0, nt = 0;                // (the largest face chain holds 2048^2 * 4 / 3 blocks, the cube 8192^2 * 8 texels: below 2^32)
    for (uint32_t l = 0; l <= MAX_LEVELS; l++) {
        L.face_first[l] = nb;
        if (l < MAX_LEVELS) L.first_texel[l] = nt;
        if (l < mip_levels) {
            const uint32_t s = size >> l;
            nb += level_blocks(s) * level_blocks(s);
            nt += 6u * s * s;
        }
    }
    L.lanes = 6u * nb;
}
// pbr_bc6h_chain_bytes: the bytes of one face's chain, 0 for a refused description
inline size_t chain_bytes(uint32_t size, uint32_t mip_levels) {
    if (!chain_ok(size, mip_levels)) return 0;
    Cube<const void*> L;
    fill(L, size, mip_levels);
    return (size_t)16 * L.face_first[mip_levels];
}

}  // namespace bc6h_chain

// the geometry of pbr_equirect_to_cube (equirect.hip): what it refuses, and the cube size and sub-sample count an import picks when its
// caller names none (pbr_equirect_default_size / _samples; structs.py restates both)
namespace equirect {

// the largest power of two <= pw / 4 — a face spans a quarter of the panorama's width, so level 0 is no finer than its source —
// clamped to [4, PBR_BC6H_MAX_SIZE]
inline uint32_t default_size(uint32_t pw) {
    uint32_t s = 4u;
    while (s < PBR_BC6H_MAX_SIZE && 2u * s <= pw / 4u) s *= 2u;
    return s;
}
// the smallest of 1, 2, 4, 8 with 4 size samples >= pw (every panorama column of the equator under at least one sub-sample); 8 if none is
inline uint32_t default_samples(uint32_t pw, uint32_t size) {
    for (uint32_t s = 1u; s < 8u; s *= 2u)
        if ((uint64_t)4u * size * s >= pw) return s;
    return 8u;
}
// what is wrong with a call's description; nullptr: nothing
inline const char* refusal(uint32_t pw, uint32_t ph, uint32_t size, uint32_t samples) {
    if (!pw || !ph || pw > PBR_EQUIRECT_MAX_W || ph > PBR_EQUIRECT_MAX_H) return "panorama size zero or above PBR_EQUIRECT_MAX_W x PBR_EQUIRECT_MAX_H";
    if (!size || size > PBR_BC6H_MAX_SIZE) return "size zero or above PBR_BC6H_MAX_SIZE";
    if (samples != 1u && samples != 2u && samples != 4u && samples != 8u) return "samples not 1, 2, 4 or 8";
    return nullptr;
}

}  // namespace equirect
