// bc6h_encode.hip — the producing half of the sky path (include/pbr_hip.h, "BC6H sky import"): what the reference's
// ResourceLoader::ImportCubeMap does after LoadCubeMap (ResourceLoader.cpp:279-299): TextureCompressor::Compress of the six faces'
// chains to DXGI_FORMAT_BC6H_UF16.  pbr_bc6h_encode_cube is the inverse of pbr_bc6h_decode_cube, same layouts on both sides.
//   k_bc6h_encode_cube   all faces and all levels in one launch, lane = block, the shape of k_bc1_encode and k_bc6h_decode_cube: the
//                        level table rides in the kernel argument and is read with static indices, the six face pointers come through
//                        a select chain, a block's texels are sixteen 16-byte loads (a lane reads 64 contiguous bytes of each of its
//                        four rows, lanes adjacent in x continue the row), the block leaves as one 16-byte store.  The texels stay in
//                        registers as 48 half codes; a fit walks the sixteen palette entries in a real loop with the sixteen texels
//                        unrolled inside it (one running minimum and one index register per texel), and the block runs six of them:
//                        the start, two refinements, and the three modes below 16 bits (the 16-bit mode's fit is the refined one).
//                        No LDS, no cross-lane traffic, no scratch.  The sixteen-lanes-per-block shape with DPP row reductions was
//                        not built: DESIGN.md section 4.
//   k_bc6h_encode_cube2  the same lane with the two-region rule on top (PBR_BC6H_ENCODE_TWO_REGION): the one-region block first, then a
//                        real loop over the 32 shapes whose counter is wave-uniform; the shape's partition pattern is a 16-bit entry
//                        of the decode rule's table, loaded by a vector load at a wave-uniform address (there is no scalar load of that
//                        width) and moved into a scalar register by v_readfirstlane; each trip is two box starts and one eight-entry fit over
//                        the sixteen texels, a texel picking its region's palette entry by its bit of the pattern.  The winner's
//                        pattern is carried per lane; two refinements and a loop over the ten modes follow.  No LDS, no scratch.
// The rule is pinned in the header, all in integers; bc6h_encode_block.hpp holds it as plain C++ that also compiles for the host
// (tools/bc6h_encode_hostcheck.cpp runs it under ASan / UBSan); tests/bc6h_encode_ref.py restates it in numpy and the kernel is held
// to that bit for bit.
#include <cstdint>

#include "pbr_internal.hpp"
#include "bc6h_encode_block.hpp"

namespace {

static_assert(sizeof(bc6h_enc::Texel) == 16 && sizeof(bc6h_enc::Block) == 16, "a texel and a block are 16-byte accesses");

__global__ __launch_bounds__(256) void k_bc6h_encode_cube(bc6h_enc::Cube L, const bc6h_enc::Texel* __restrict__ cube) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= L.lanes) return;
    bc6h_enc::encode_lane(L, g, cube);
}

__global__ __launch_bounds__(256, 2) void k_bc6h_encode_cube2(bc6h_enc::Cube L, const bc6h_enc::Texel* __restrict__ cube) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= L.lanes) return;
    bc6h_enc::encode_lane<true>(L, g, cube);
}

// both entry points; a refusal carries the name of the one that was called
pbr_status encode_cube(pbr_ctx* ctx, const char* who, const float* cube_rgba, uint32_t size, uint32_t mip_levels, void* const face_blocks_out[6],
                       uint32_t flags) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_CHECK(ctx, who, (flags & ~PBR_BC6H_ENCODE_TWO_REGION) != 0 ? "unknown flag" : nullptr);
    PBR_CHECK(ctx, who, face_blocks_out && cube_rgba ? nullptr : "null pointer");
    PBR_CHECK(ctx, who, bc6h_chain::refusal(size, mip_levels));
    PBR_CHECK(ctx, who, (pbr::addr(cube_rgba) & 15u) == 0 ? nullptr : "cube_rgba not 16-byte aligned");
    PBR_CHECK(ctx, who, bc6h_chain::faces_refusal(face_blocks_out));
    bc6h_enc::Cube L;
    for (int f = 0; f < 6; f++) L.face[f] = face_blocks_out[f];
    bc6h_chain::fill(L, size, mip_levels);
    const bool two = (flags & PBR_BC6H_ENCODE_TWO_REGION) != 0;
    hipLaunchKernelGGL(two ? k_bc6h_encode_cube2 : k_bc6h_encode_cube, dim3((L.lanes + 255u) / 256u), dim3(256), 0, ctx->stream, L,
                       reinterpret_cast<const bc6h_enc::Texel*>(cube_rgba));
    return pbr::launched(ctx, two ? "k_bc6h_encode_cube2" : "k_bc6h_encode_cube");
}

}  // namespace

extern "C" {

pbr_status pbr_bc6h_encode_cube_ex(pbr_ctx* ctx, const float* cube_rgba, uint32_t size, uint32_t mip_levels, void* const face_blocks_out[6],
                                   uint32_t flags) {
    return encode_cube(ctx, "pbr_bc6h_encode_cube_ex", cube_rgba, size, mip_levels, face_blocks_out, flags);
}

pbr_status pbr_bc6h_encode_cube(pbr_ctx* ctx, const float* cube_rgba, uint32_t size, uint32_t mip_levels, void* const face_blocks_out[6]) {
    return encode_cube(ctx, "pbr_bc6h_encode_cube", cube_rgba, size, mip_levels, face_blocks_out, 0u);
}

}  // extern "C"
