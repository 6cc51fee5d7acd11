// gbuffer_encode.hpp — gbuffer.hlsl::ps_main's output encode (gbuffer.hlsl:144-146), shared by k_gbuffer_encode (raster.hip,
// per-pixel material planes) and k_rs_raster (gbuffer_raster.hip, constant per-draw materials).  Both translation units are
// built with -ffp-contract=off: the gamma / octahedral results feed UNORM8 rounding.
// Included inside each user's anonymous namespace, after pbr_device.hpp (sign_custom) and `using namespace pbr`.
#pragma once

__device__ __forceinline__ uint32_t unorm8(float x) { return (uint32_t)floorf(saturatef(x) * 255.0f + 0.5f); }
// decode_gamma (global.hlsli:73-77): pow(c, 2.2) the way the shader compiler lowers it, exp2(2.2 * log2(c)) on
// the transcendental unit (v_log_f32 / v_exp_f32, 1 ULP each).  The result only feeds an 8-bit UNORM target:
// relative error < 1e-6 moves a value across a rounding boundary on ~1e-4 of the texels (by one step).
// pow(0) = 0, pow(negative) = NaN -> saturate -> 0, like the libm formulation.
__device__ __forceinline__ float decode_gamma(float c) {
    return __builtin_amdgcn_exp2f(2.2f * __builtin_amdgcn_logf(c));
}

// a = (albedo.rgb as authored (gamma space), emission), b = (normal_ws.xyz, roughness), c = (metallic, ambient occlusion, -, -)
// (float4 each) -> declares pa, pb, pc: the three RGBA8 targets (global.hlsli:73-77,101-133; formats DeferredPipeline.h:107-109).
// Statements, not a function: behind a call boundary the compiler vectorises k_gbuffer_encode differently.
#define PBR_GBUFFER_ENCODE(a, b, c, pa, pb, pc)                                                                                   \
    /* decode_gamma, global.hlsli:73-77 */                                                                                        \
    const uint32_t pa = unorm8(decode_gamma((a).x)) | (unorm8(decode_gamma((a).y)) << 8) | (unorm8(decode_gamma((a).z)) << 16) | \
                        (unorm8((a).w) << 24);                                                                                    \
    /* pack_normal(normalize(n)), global.hlsli:117-128 */                                                                        \
    V3 n = normalize3_exact(v3((b).x, (b).y, (b).z));                                                                            \
    const float sum = fabsf(n.x) + fabsf(n.y) + fabsf(n.z);                                                                       \
    float dx = n.x / sum, dy = n.y / sum;                                                                                         \
    const float dz = n.z / sum;                                                                                                   \
    if (dz < 0.0f) {                                                                                                              \
        const float nx = sign_custom(dx) * (1.0f - fabsf(dy));                                                                    \
        const float ny = sign_custom(dy) * (1.0f - fabsf(dx));                                                                    \
        dx = nx; dy = ny;                                                                                                         \
    }                                                                                                                             \
    const uint32_t pb = unorm8(dx * 0.5f + 0.5f) | (unorm8(dy * 0.5f + 0.5f) << 8) | (255u << 16);                               \
    const uint32_t pc = unorm8((b).w) | (unorm8((c).x) << 8) | (unorm8((c).y) << 16);
