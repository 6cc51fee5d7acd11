// bc6h_decode.hip — the reference's load-time decode of a sky asset on the GPU (include/pbr_hip.h, "BC6H sky cubes"): a CubeMapResource
// holds six DXGI_FORMAT_BC6H_UF16 chains (TextureCompression.h:13-14, ResourceDef.cpp:187-219) that DirectX::Decompress expands when
// the file is read; pbr_bc6h_decode_cube expands them into the fp32 RGBA cube chain every consumer here takes (pbr_cube_f32).
//   k_bc6h_decode_cube   all faces and all levels in one launch, lane = block.  The block is one 16-byte load (a wave reads 1 KiB of
//                        consecutive blocks) kept as two 64-bit words; a switch on the mode runs that mode's header as straight-line
//                        bit-field extracts (every field position is a template constant: the four words never become an indexed
//                        array), applies the delta transform and unquantizes; the code after the switch is shared: per texel one
//                        64-bit shift of the upper word gives the index (all index bits lie there), a shift of a packed constant the
//                        weight, then three interpolations, and each texel leaves as one 16-byte store — a lane writes the block's
//                        rows as 4 x 64 bytes, lanes adjacent in x cover a contiguous run of a row.  No LDS, no cross-lane traffic.
//                        A wave runs every mode its lanes hold: random blocks are the worst case, a real sky uses few modes per
//                        neighbourhood.
// The rule is pinned in the header; tests/bc6h_ref.py restates it in numpy (held to a third-party decoder on the CPU) and the kernel
// is held to that bit for bit.
#include <cstdint>

#include "pbr_internal.hpp"
#include "pbr_device.hpp"
#include "bc6h_decode_block.hpp"     // the mode tables, read_header / endpoints<M>, PARTITION, the anchor and weight constants

namespace {

using namespace bc6h_dec;

constexpr uint32_t BC6H_MAX_LEVELS = 14;    // floor(log2(PBR_BC6H_MAX_SIZE)) + 1
static_assert((1u << (BC6H_MAX_LEVELS - 1)) == PBR_BC6H_MAX_SIZE, "levels of the largest cube");

struct Bc6hCube {
    const uint4* face[6];
    uint32_t face_first[BC6H_MAX_LEVELS + 1];   // blocks of one face in front of the level; [mips] = one face's blocks
    uint32_t first_texel[BC6H_MAX_LEVELS];      // pbr_cube_mip_offset of the level
    uint32_t size, mips;
    uint32_t lanes;                             // 6 x one face's blocks
};

// lane = block; the lanes of a level are face after face, the face's blocks row-major
__global__ __launch_bounds__(256) void k_bc6h_decode_cube(Bc6hCube L, float4* __restrict__ out) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= L.lanes) return;
    uint32_t l = 0, ff = 0, ft = 0;
#pragma unroll
    for (uint32_t k = 1; k < BC6H_MAX_LEVELS; k++) {          // (static indices: the table stays in scalar registers)
        if (k < L.mips && g >= 6u * L.face_first[k]) { l = k; ff = L.face_first[k]; ft = L.first_texel[k]; }
    }
    const uint32_t s = L.size >> l, bw = max(1u, (s + 3u) >> 2), nb = bw * bw;
    const uint32_t k = g - 6u * ff, f = k / nb, r = k - f * nb, by = r / bw, bx = r - by * bw;
    const uint4* src = f == 0 ? L.face[0] : f == 1 ? L.face[1] : f == 2 ? L.face[2] : f == 3 ? L.face[3] : f == 4 ? L.face[4] : L.face[5];
    const uint4 q = src[ff + r];
    const uint64_t lo = q.x | ((uint64_t)q.y << 32), hi = q.z | ((uint64_t)q.w << 32);

    uint32_t e[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    const uint32_t mode = (q.x & 2u) ? q.x & 31u : q.x & 3u;
    bool two = false;
    switch (mode) {
        case 0x00: endpoints<0x00>(lo, hi, e); two = true; break;
        case 0x01: endpoints<0x01>(lo, hi, e); two = true; break;
        case 0x02: endpoints<0x02>(lo, hi, e); two = true; break;
        case 0x06: endpoints<0x06>(lo, hi, e); two = true; break;
        case 0x0a: endpoints<0x0a>(lo, hi, e); two = true; break;
        case 0x0e: endpoints<0x0e>(lo, hi, e); two = true; break;
        case 0x12: endpoints<0x12>(lo, hi, e); two = true; break;
        case 0x16: endpoints<0x16>(lo, hi, e); two = true; break;
        case 0x1a: endpoints<0x1a>(lo, hi, e); two = true; break;
        case 0x1e: endpoints<0x1e>(lo, hi, e); two = true; break;
        case 0x03: endpoints<0x03>(lo, hi, e); break;
        case 0x07: endpoints<0x07>(lo, hi, e); break;
        case 0x0b: endpoints<0x0b>(lo, hi, e); break;
        case 0x0f: endpoints<0x0f>(lo, hi, e); break;
        default: break;                                       // 0x13, 0x17, 0x1b, 0x1f are reserved: every endpoint 0, rgb = 0
    }

    // indices: 3 bits from block bit 82 (two regions) or 4 bits from bit 65, an anchor texel one bit fewer; all in `hi`
    const uint32_t shape = (uint32_t)(hi >> 13) & 31u;        // bits 77 .. 81
    const uint32_t pattern = two ? (uint32_t)PARTITION[shape] : 0u;
    const uint32_t anchor = !two ? 16u : shape < 16u ? 15u : (uint32_t)(ANCHOR_16_31 >> (4u * (shape - 16u))) & 15u;
    const uint32_t ib = two ? 3u : 4u, base = two ? 18u : 1u;
    float4* dst = out + ft + ((size_t)f * s + 4u * by) * s + 4u * bx;
#pragma unroll
    for (uint32_t t = 0; t < 16u; t++) {
        const uint32_t x = t & 3u, y = t >> 2;
        const uint32_t start = base + ib * t - (t > 0u ? 1u : 0u) - (t > anchor ? 1u : 0u);
        const uint32_t width = ib - ((t == 0u || t == anchor) ? 1u : 0u);
        const uint32_t idx = (uint32_t)(hi >> start) & ((1u << width) - 1u);
        const uint32_t w = (uint32_t)((two ? WEIGHTS3 : idx < 8u ? WEIGHTS4_LO : WEIGHTS4_HI) >> (8u * (idx & 7u))) & 255u;
        const bool second = (pattern >> t) & 1u;
        float c[3];
#pragma unroll
        for (uint32_t ch = 0; ch < 3u; ch++) {
            const uint32_t a = second ? e[6u + ch] : e[ch], b = second ? e[9u + ch] : e[3u + ch];
            const uint32_t v = (a * (64u - w) + b * w + 32u) >> 6;            // a, b <= 0xffff: below 2^22
            const uint16_t h = (uint16_t)((v * 31u) >> 6);                    // <= 0x7bff: finite
            c[ch] = (float)__builtin_bit_cast(_Float16, h);                   // exact, subnormal halves included
        }
        if (4u * bx + x < s && 4u * by + y < s) dst[(size_t)y * s + x] = make_float4(c[0], c[1], c[2], 1.0f);
    }
}

uint32_t max_levels(uint32_t size) {
    uint32_t n = 0;
    while (size) { n++; size >>= 1; }
    return n;
}
uint32_t level_blocks(uint32_t s) { const uint32_t b = (s + 3u) / 4u; return b ? b : 1u; }
bool chain_ok(uint32_t size, uint32_t mip_levels) {
    return size >= 4u && size <= PBR_BC6H_MAX_SIZE && (size & 3u) == 0 && mip_levels >= 1u && mip_levels <= max_levels(size);
}

}  // namespace

extern "C" {

size_t pbr_bc6h_chain_bytes(uint32_t size, uint32_t mip_levels) {
    if (!chain_ok(size, mip_levels)) return 0;
    size_t blocks = 0;
    for (uint32_t l = 0; l < mip_levels; l++) blocks += (size_t)level_blocks(size >> l) * level_blocks(size >> l);
    return 16u * blocks;
}

pbr_status pbr_bc6h_decode_cube(pbr_ctx* ctx, const void* const face_blocks[6], uint32_t size, uint32_t mip_levels, float* out_rgba) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, face_blocks && out_rgba, "pbr_bc6h_decode_cube: null pointer");
    PBR_REQUIRE(ctx, chain_ok(size, mip_levels),
                "pbr_bc6h_decode_cube: size 0, not a multiple of 4 or above PBR_BC6H_MAX_SIZE, or mip_levels 0 or above floor(log2(size)) + 1");
    PBR_REQUIRE(ctx, (pbr::addr(out_rgba) & 15u) == 0, "pbr_bc6h_decode_cube: out_rgba not 16-byte aligned");
    Bc6hCube L;
    for (int f = 0; f < 6; f++) {
        PBR_REQUIRE(ctx, face_blocks[f], "pbr_bc6h_decode_cube: null face pointer");
        PBR_REQUIRE(ctx, (pbr::addr(face_blocks[f]) & 15u) == 0, "pbr_bc6h_decode_cube: face blocks not 16-byte aligned");
        L.face[f] = static_cast<const uint4*>(face_blocks[f]);
    }
    L.size = size; L.mips = mip_levels;
    uint32_t nb = 0;                              // (the largest face chain holds 2048^2 * 4 / 3 blocks, the cube 8192^2 * 8 texels: below 2^32)
    for (uint32_t l = 0; l <= BC6H_MAX_LEVELS; l++) {
        L.face_first[l] = nb;
        if (l < BC6H_MAX_LEVELS) L.first_texel[l] = (uint32_t)pbr::cube_mip_offset(size, l < mip_levels ? l : mip_levels);
        if (l < mip_levels) nb += level_blocks(size >> l) * level_blocks(size >> l);
    }
    L.lanes = 6u * nb;
    hipLaunchKernelGGL(k_bc6h_decode_cube, dim3((L.lanes + 255u) / 256u), dim3(256), 0, ctx->stream, L, reinterpret_cast<float4*>(out_rgba));
    return pbr::launched(ctx, "k_bc6h_decode_cube");
}

}  // extern "C"
