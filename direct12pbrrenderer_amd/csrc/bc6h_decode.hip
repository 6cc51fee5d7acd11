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
#include "tex_chain.hpp"
#include "bc6h_decode_block.hpp"     // the mode switch, the per-texel weight and the partition tables, shared with the in-place sky resolve

namespace {

using namespace bc6h_dec;

using Bc6hCube = bc6h_chain::Cube<const uint4*>;

// lane = block; the lanes of a level are face after face, the face's blocks row-major
__global__ __launch_bounds__(256) void k_bc6h_decode_cube(Bc6hCube L, float4* __restrict__ out) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= L.lanes) return;
    uint32_t l = 0, ff = 0, ft = 0;
#pragma unroll
    for (uint32_t k = 1; k < bc6h_chain::MAX_LEVELS; k++) {          // (static indices: the table stays in scalar registers)
        if (k < L.mips && g >= 6u * L.face_first[k]) { l = k; ff = L.face_first[k]; ft = L.first_texel[k]; }
    }
    const uint32_t s = L.size >> l, bw = max(1u, (s + 3u) >> 2), nb = bw * bw;
    const uint32_t k = g - 6u * ff, f = k / nb, r = k - f * nb, by = r / bw, bx = r - by * bw;
    const uint4* src = f == 0 ? L.face[0] : f == 1 ? L.face[1] : f == 2 ? L.face[2] : f == 3 ? L.face[3] : f == 4 ? L.face[4] : L.face[5];
    const uint4 q = src[ff + r];
    const uint64_t lo = q.x | ((uint64_t)q.y << 32), hi = q.z | ((uint64_t)q.w << 32);

    uint32_t e[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    const bool two = mode_endpoints(lo, hi, e);
    // (the three lines of bc6h_dec::header(), kept here as text: from a shared function, by reference or by value, both this kernel's
    // and k_skybox_bc6h's instruction streams came out different)
    const uint32_t shape = (uint32_t)(hi >> 13) & 31u;        // bits 77 .. 81
    const uint32_t pattern = two ? (uint32_t)PARTITION[shape] : 0u;
    const uint32_t anchor = !two ? 16u : shape < 16u ? 15u : (uint32_t)(ANCHOR_16_31 >> (4u * (shape - 16u))) & 15u;
    float4* dst = out + ft + ((size_t)f * s + 4u * by) * s + 4u * bx;
#pragma unroll
    for (uint32_t t = 0; t < 16u; t++) {
        const uint32_t x = t & 3u, y = t >> 2;
        const uint32_t w = texel_weight(hi, two, anchor, t);
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

}  // namespace

extern "C" {

size_t pbr_bc6h_chain_bytes(uint32_t size, uint32_t mip_levels) { return bc6h_chain::chain_bytes(size, mip_levels); }

pbr_status pbr_bc6h_decode_cube(pbr_ctx* ctx, const void* const face_blocks[6], uint32_t size, uint32_t mip_levels, float* out_rgba) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, face_blocks && out_rgba, "pbr_bc6h_decode_cube: null pointer");
    PBR_CHECK(ctx, "pbr_bc6h_decode_cube", bc6h_chain::refusal(size, mip_levels));
    PBR_REQUIRE(ctx, (pbr::addr(out_rgba) & 15u) == 0, "pbr_bc6h_decode_cube: out_rgba not 16-byte aligned");
    PBR_CHECK(ctx, "pbr_bc6h_decode_cube", bc6h_chain::faces_refusal(face_blocks));
    Bc6hCube L;
    for (int f = 0; f < 6; f++) L.face[f] = static_cast<const uint4*>(face_blocks[f]);
    bc6h_chain::fill(L, size, mip_levels);
    hipLaunchKernelGGL(k_bc6h_decode_cube, dim3((L.lanes + 255u) / 256u), dim3(256), 0, ctx->stream, L, reinterpret_cast<float4*>(out_rgba));
    return pbr::launched(ctx, "k_bc6h_decode_cube");
}

}  // extern "C"
