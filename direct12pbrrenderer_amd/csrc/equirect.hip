// equirect.hip — an equirectangular (latitude-longitude) HDR panorama resampled into level 0 of a sky cube (include/pbr_hip.h,
// "Equirectangular panoramas"): the step in front of pbr_cube_gen_mips, pbr_sh9_project and pbr_bc6h_encode_cube_ex for a sky that
// arrives as ONE .hdr file instead of six faces.  The reference takes faces only (ResourceLoader.cpp:408-428); the rule is this
// project's own and pinned in the header, tests/equirect_ref.py restates it in numpy.
//   k_equirect_to_cube<SAMPLES, RGBE>   all six faces in one launch; block = a 16 x 16 tile of one face, lane = output texel, so the
//                        lanes of a wave (four rows of 16) gather neighbouring panorama texels: away from the poles a tile's taps
//                        fall into a patch of about (16 pw / 4 size) x (16 ph / 2 size) texels.  Per sub-sample: one IEEE divide per
//                        axis (hoisted out of the inner loop for y), two atan2f, a sqrt, four taps (16-byte loads, or 4-byte loads
//                        decoded in place for an RGBE source) and nine fmaf.  One 16-byte store per lane, contiguous along x.  No LDS,
//                        no cross-lane traffic.  SAMPLES and the source format are template parameters: eight instantiations.
// #pragma clang fp contract(off) pins the coordinate chain: the two source formats then run the same operations on the same
// coordinates whatever the optimiser fuses elsewhere, which is what makes their outputs bit-identical.
#include <cstdint>

#include "pbr_internal.hpp"
#include "pbr_device.hpp"
#include "tex_chain.hpp"

namespace {

using namespace pbr;

constexpr float INV_TWO_PI = 0.15915494309189535f;   // fp32 nearest of 1 / (2 pi)
constexpr float INV_PI     = 0.3183098861837907f;    // fp32 nearest of 1 / pi

struct EquirectParams {
    uint32_t pw, ph, size;
};

// one tap: the texel as it is (fp32 source) or pbr_rgbe_decode's rule where it is fetched (k_rgbe_decode, raster.hip: exact)
template <bool RGBE>
__device__ __forceinline__ V3 equirect_tap(const void* __restrict__ pano, uint32_t pw, uint32_t row, uint32_t col) {
    const size_t i = (size_t)row * pw + col;
    if constexpr (RGBE) {
        const uint32_t v = static_cast<const uint32_t*>(pano)[i];
        const int e = (int)(v >> 24);
        const float scale = e ? ldexpf(1.0f, e - 136) : 0.0f;
        return v3((float)(v & 255u) * scale, (float)((v >> 8) & 255u) * scale, (float)((v >> 16) & 255u) * scale);
    } else {
        const float4 v = static_cast<const float4*>(pano)[i];
        return v3(v.x, v.y, v.z);
    }
}
__device__ __forceinline__ V3 equirect_lerp(V3 p, V3 q, float w) {
    return v3(__builtin_fmaf(w, q.x - p.x, p.x), __builtin_fmaf(w, q.y - p.y, p.y), __builtin_fmaf(w, q.z - p.z, p.z));
}

template <int SAMPLES, bool RGBE>
__global__ __launch_bounds__(256) void k_equirect_to_cube(EquirectParams P, const void* __restrict__ pano, float4* __restrict__ out) {
#pragma clang fp contract(off)
    const uint32_t x = blockIdx.x * 16u + (threadIdx.x & 15u), y = blockIdx.y * 16u + (threadIdx.x >> 4), f = blockIdx.z;
    if (x >= P.size || y >= P.size) return;
    const int n = (int)(P.size * (uint32_t)SAMPLES);          // <= 8192 * 8: every numerator below is exact in fp32
    const float fn = (float)n, fpw = (float)P.pw, fph = (float)P.ph;
    const int pw = (int)P.pw, ph = (int)P.ph;
    V3 acc = v3(0.0f, 0.0f, 0.0f);
#pragma unroll 1
    for (int j = 0; j < SAMPLES; j++) {
        const float b = (float)(2 * ((int)y * SAMPLES + j) + 1 - n) / fn;
#pragma unroll 1
        for (int i = 0; i < SAMPLES; i++) {
            const float a = (float)(2 * ((int)x * SAMPLES + i) + 1 - n) / fn;
            const V3 d = cube_dir_raw(f, a, b);
            const float lambda = (d.x == 0.0f && d.z == 0.0f) ? 0.0f : atan2f(d.x, d.z);
            const float theta = atan2f(sqrtf(d.x * d.x + d.z * d.z), d.y);
            const float s = (lambda * INV_TWO_PI + 0.5f) * fpw - 0.5f;
            const float t = (theta * INV_PI) * fph - 0.5f;
            const float sf = floorf(s), tf = floorf(t);
            const float fx = s - sf, fy = t - tf;
            // s lies in [-1/2, pw]: one conditional step wraps either tap; the clamp keeps every address inside the panorama whatever
            // the coordinate chain returns
            int x0 = (int)sf, x1 = x0 + 1;
            x0 += x0 < 0 ? pw : 0;   x0 -= x0 >= pw ? pw : 0;
            x1 += x1 < 0 ? pw : 0;   x1 -= x1 >= pw ? pw : 0;
            x0 = clampi(x0, 0, pw - 1);
            x1 = clampi(x1, 0, pw - 1);
            const int y0 = clampi((int)tf, 0, ph - 1), y1 = clampi((int)tf + 1, 0, ph - 1);
            const V3 c00 = equirect_tap<RGBE>(pano, P.pw, (uint32_t)y0, (uint32_t)x0);
            const V3 c10 = equirect_tap<RGBE>(pano, P.pw, (uint32_t)y0, (uint32_t)x1);
            const V3 c01 = equirect_tap<RGBE>(pano, P.pw, (uint32_t)y1, (uint32_t)x0);
            const V3 c11 = equirect_tap<RGBE>(pano, P.pw, (uint32_t)y1, (uint32_t)x1);
            const V3 c = equirect_lerp(equirect_lerp(c00, c10, fx), equirect_lerp(c01, c11, fx), fy);
            acc = acc + c;
        }
    }
    constexpr float INV = 1.0f / (float)(SAMPLES * SAMPLES);   // a power of two: exact
    out[((size_t)f * P.size + y) * P.size + x] = make_float4(acc.x * INV, acc.y * INV, acc.z * INV, 1.0f);
}

template <bool RGBE>
void launch_equirect(pbr_ctx* ctx, const EquirectParams& P, uint32_t samples, const void* pano, float4* out) {
    const dim3 grid((P.size + 15u) / 16u, (P.size + 15u) / 16u, 6u), block(256);
    switch (samples) {
        case 1: hipLaunchKernelGGL((k_equirect_to_cube<1, RGBE>), grid, block, 0, ctx->stream, P, pano, out); break;
        case 2: hipLaunchKernelGGL((k_equirect_to_cube<2, RGBE>), grid, block, 0, ctx->stream, P, pano, out); break;
        case 4: hipLaunchKernelGGL((k_equirect_to_cube<4, RGBE>), grid, block, 0, ctx->stream, P, pano, out); break;
        default: hipLaunchKernelGGL((k_equirect_to_cube<8, RGBE>), grid, block, 0, ctx->stream, P, pano, out); break;
    }
}

}  // namespace

extern "C" {

uint32_t pbr_equirect_default_size(uint32_t pw) { return equirect::default_size(pw); }
uint32_t pbr_equirect_default_samples(uint32_t pw, uint32_t size) { return equirect::default_samples(pw, size); }

pbr_status pbr_equirect_to_cube(pbr_ctx* ctx, const void* pano, uint32_t pw, uint32_t ph, float* cube_level0, uint32_t size,
                                uint32_t samples, uint32_t flags) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, pano && cube_level0, "pbr_equirect_to_cube: null pointer");
    PBR_REQUIRE(ctx, (flags & ~PBR_EQUIRECT_SRC_RGBE) == 0, "pbr_equirect_to_cube: unknown flag");
    PBR_CHECK(ctx, "pbr_equirect_to_cube", equirect::refusal(pw, ph, size, samples));
    const bool rgbe = (flags & PBR_EQUIRECT_SRC_RGBE) != 0;
    PBR_REQUIRE(ctx, (pbr::addr(cube_level0) & 15u) == 0, "pbr_equirect_to_cube: cube_level0 not 16-byte aligned");
    PBR_REQUIRE(ctx, (pbr::addr(pano) & (rgbe ? 3u : 15u)) == 0, "pbr_equirect_to_cube: pano not aligned to its texel (16 bytes fp32, 4 bytes RGBE)");
    const EquirectParams P{pw, ph, size};
    if (rgbe) launch_equirect<true>(ctx, P, samples, pano, reinterpret_cast<float4*>(cube_level0));
    else      launch_equirect<false>(ctx, P, samples, pano, reinterpret_cast<float4*>(cube_level0));
    return pbr::launched(ctx, "k_equirect_to_cube");
}

}  // extern "C"
