// shade.hip — deferred Cook-Torrance shade of a G-buffer tile (deferred_shading.hlsl:91-192).
//
// Replaces the stencil-masked full-screen draw of DeferredShadingPass::Execute
// (DeferredPipeline.cpp:187-206).  MI355X mapping:
//  * one lane per pixel, a wave = 64 consecutive pixels of a row: every G-buffer plane is read as
//    one 256-byte (RGBA8 / depth) or 64-byte (stencil) coalesced segment per wave, the half4 output
//    is one 512-byte store; a block walks SHADE_ROWS rows after staging its tables once;
//  * the light table is staged in LDS as nine structure-of-arrays planes (position, colour * intensity, attenuation):
//    the same component of two lights lands in an adjacent VGPR pair straight from two ds_read_b32;
//  * the light lists of the clusters the block can touch are staged in LDS as LDS byte addresses of the lights (one
//    dword each: a trip's two entries are ONE ds_read_b64, each address in its own register), so the divergent per-lane
//    list walk is an LDS read, not a global gather (blocks that span too many cluster tiles — tiny render targets —
//    fall back to the global list);
//  * the env chain is sampled from its padded layout (pbr_env_pad): no seam branches, each bilinear row is one
//    16-byte load;
//  * with 256 lights the kernel is FP32-VALU-issue-bound (46 packed + 4 transcendental instructions per pair of lights and
//    one compare + one pointer step per WALK_TRIPS pairs, ~430 per pixel around the loop), not HBM-bound.
#include <cstring>
#include <type_traits>
#include "pbr_internal.hpp"
#include "pbr_device.hpp"

using namespace pbr;

struct ShadeParams {
    pbr_sh_pack sh;
    float InvView[9];      // 3x3 part, row-major
    float CameraPos[3];
    float Near, Far;
    float near_width, near_height;   // 2 Near tan(Fov/2) [* Ratio]  (vs_main :94-95), host libm
    float log_far_near;              // log(Far/Near) of ClusterIndex (clustered.hlsli:53), host libm
    float inv_near, slice_k;         // 1 / Near and PBR_CLUSTER_Z / log2(Far/Near) (host, from double): the slice index's quick estimate
    uint32_t x0, y0, w, h, full_w, full_h;
    const uint32_t* A;
    const uint32_t* B;
    const uint32_t* C;
    const float* depth;
    const uint8_t* stencil;
    uint32_t pitch;
    const pbr_half* lut;
    const float* lut_fold;   // LUTFOLD instantiations: the x-folded LUT (pbr_lut_fold_x) instead of `lut`
    uint32_t lut_res;
    const pbr_half* env;   // padded layout
    uint32_t env_size, env_mips;
    uint32_t env_mip_off[16];   // texel offset of each padded mip (host-computed)
    const pbr_cluster* clusters;
    const pbr_light* lights;
    pbr_half* hdr;
    uint32_t hdr_pitch;
    float* hdr_f32;        // F32OUT instantiations only (pbr_deferred_shade_f32): the colour BEFORE the fp16 store
};

// ViewSpaceDepth (pbr_device.hpp: view_space_depth, the exact form) with v_rcp for the division (<= 2 ulp from the IEEE result): for consumers that are continuous in z_vs
__device__ __forceinline__ float view_space_depth_quick(float d, float near_z, float far_z) {
#pragma clang fp contract(off)
    const float range = far_z - near_z;
    const float prod = d * range;
    const float den = far_z - prod;
    return (near_z * far_z) * rcp(den);
}

// ------------------------------------------------------------------------------------------------
// "Padded" env chain = the footprint layout of pbr_device.hpp::env_padded_mip_offset: entry (face, yq, xq), xq, yq in
// [0, s], holds the four texels of the bilinear footprint whose origin is tap (xq-1, yq-1), each resolved by the
// seamless-cube rule.  One thread per stored texel.
__global__ __launch_bounds__(256) void k_env_pad(const pbr_half* __restrict__ src, pbr_half* __restrict__ dst, int s) {
    const int sq = s + 1;
    const size_t n = (size_t)6 * sq * sq * 4;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int k = (int)(t & 3), xq = (int)((t >> 2) % sq), yq = (int)(((t >> 2) / sq) % sq);
    uint32_t face = (uint32_t)((t >> 2) / ((size_t)sq * sq));
    int x = xq - 1 + (k & 1), y = yq - 1 + (k >> 1);
    const bool xo = (x < 0) | (x >= s), yo = (y < 0) | (y >= s);
    if (xo | yo) {   // same rule as pbr::cube_fetch_seamless / the oracle
        if (xo & yo) y = clampi(y, 0, s - 1);
        const float uu = 2.0f * ((float)x + 0.5f) / (float)s - 1.0f;
        const float vv = 2.0f * ((float)y + 0.5f) / (float)s - 1.0f;
        float u2, v2;
        cube_face_uv(cube_dir_raw(face, uu, vv), face, u2, v2);
        x = clampi((int)floorf(u2 * (float)s), 0, s - 1);
        y = clampi((int)floorf(v2 * (float)s), 0, s - 1);
    }
    reinterpret_cast<H4*>(dst)[t] = reinterpret_cast<const H4*>(src)[((size_t)face * s + y) * s + x];
}

// Light table in LDS, structure-of-arrays: 9 planes of LSTRIDE floats
//   0..2 position, 3..5 color*intensity, 6..8 attenuation C0,C1,C2
// SoA (not 48-byte records) so that the SAME component of two different lights lands in an adjacent
// VGPR pair straight from two ds_read_b32 — the operand shape v_pk_*_f32 wants — with no repacking
// moves; the plane stride is a compile-time constant so the plane offset rides in the DS offset field.
constexpr int LIGHT_PLANES = 9;

// Which pixels of the tile a launch shades: up to SHADE_MAX_RECTS rectangles (tile-local), walked by ONE 1-D grid — a
// whole tile is one rectangle; the overlapped multi-GPU frame shades the tile's border ring (<= 4 rectangles) in one
// launch and its core in another.  Per rectangle the two-zone schedule of the kernel applies.
constexpr int SHADE_MAX_RECTS = 5;
struct ShadeRects {
    uint32_t n, rows_big, rows_small;   // rows of a long / of a short block (<= SHADE_ROWS)
    uint32_t x0[SHADE_MAX_RECTS], y0[SHADE_MAX_RECTS], w[SHADE_MAX_RECTS], h[SHADE_MAX_RECTS];
    uint32_t cols[SHADE_MAX_RECTS], nb_big[SHADE_MAX_RECTS], first[SHADE_MAX_RECTS + 1];   // first block of rect r; [n] = total
};

constexpr int SHADE_BLOCK = 256;
constexpr int SHADE_ROWS = 8;          // most rows of 256 pixels one block walks after staging its tables (12: no change, 16: +3 %, round 5)
constexpr int MAX_STAGED_TILES = 12;   // cluster (x,y) tiles whose 8 z-slices may be staged per block
// staged list: count, pad, 32 u16 indices = 34 halfwords (68 B) per cluster
constexpr int LIST_STRIDE = 34;         // dwords per staged cluster list: count, pad, 32 entries (8-byte aligned pairs)
constexpr int WALK_TRIPS = SHADE_WALK_TRIPS;   // (defined in pbr_device.hpp: the cull pads the shade tables' lists with it too) trips (pairs of lights) per pointer step and compare of the staged walk; lists are padded to 2 * WALK_TRIPS entries
static_assert(WALK_TRIPS == 2 || WALK_TRIPS == 4, "a staging thread converts four entries: the padded length must be a multiple of four that divides 32");

typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 f2s(float a) { return f2{a, a}; }
__device__ __forceinline__ f2 max2(f2 a, f2 b) { return f2{fmaxf(a.x, b.x), fmaxf(a.y, b.y)}; }
typedef __attribute__((address_space(3))) const float lds_cf;   // a float in LDS: 32-bit addresses, ds_read with an immediate plane offset
__device__ __forceinline__ f2 rsq2(f2 a) { return f2{rsq(a.x), rsq(a.y)}; }
__device__ __forceinline__ f2 rcp2(f2 a) { return f2{rcp(a.x), rcp(a.y)}; }

// v_pk_mul_f32 with the clamp output modifier: clamp(a * b, 0, 1) on both halves, free of charge.  Used for the
// cosines N.L and N.H, which the shader clamps from below with max(., 0) and which cannot exceed 1 except by a
// rounding error of normalised vectors (1 + 1e-7 becomes 1).
// The s_nop on either side are REQUIRED: gfx950 needs one wait state between a transcendental (v_rsq / v_rcp) or a
// packed-fp32 instruction and a VALU instruction that reads its result.  The compiler inserts those wait states for
// the code it schedules, but it cannot see into an asm statement: without them this instruction consumed a v_rsq result
// issued immediately before it and read the register's OLD value in the high half (second light of the pair) — found
// as a parity failure that came and went with instruction scheduling.
__device__ __forceinline__ f2 mul2_sat(f2 a, f2 b) {
    f2 r;
    asm("s_nop 0\n\tv_pk_mul_f32 %0, %1, %2 clamp\n\ts_nop 0" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// {0, 0} in a register pair with one instruction.  (s_nop: the wait state a packed-fp32 consumer of the result needs, which the
// compiler cannot insert around asm — see mul2_sat.)
__device__ __forceinline__ f2 zero2() {
    f2 r;
    asm("v_pk_mov_b32 %0, 0, 0\n\ts_nop 0" : "=v"(r));
    return r;
}

struct alignas(8) H4x2 { H4 a, b; };   // two x-adjacent half4 texels (16 bytes, 8-byte aligned)
struct alignas(4) H2x2 { H2 a, b; };   // two x-adjacent LUT texels (8 bytes, 4-byte aligned)

// The x side of the LUT's bilinear sample (clamp addressing, Q5) is a function of the roughness byte and the LUT alone.  lut_x_side:
// the row pair (xb, xb + 1) always lies inside the row; where the sampler's clamp makes both taps the SAME texel (the first / last
// half texel) the weight is moved onto it (0 or 1) instead of selecting texels.  Roughness lies in [0, 1] (UNORM8): no NaN / range
// guard; x.8 fixed-point snap as in pbr_device.hpp::bilinear_coord.  lut_row_pair / lut_x_lerp: the pair of one row and its lerp (two
// v_fma_mix_f32 per channel).  The pixel evaluates them per sample; pbr_lut_fold_x evaluates the SAME functions once per (row,
// roughness byte) into the folded table, whose entries are therefore the pixel's own fp32 values.
struct LutX { int xb; float fx, wx0; };
__device__ __forceinline__ LutX lut_x_side(float roughness, int lr) {
    const float xs = snap8(roughness * (float)lr) - 0.5f;
    const float xfl = floorf(xs);
    const int xi = (int)xfl;
    LutX r;
    r.xb = clampi(xi, 0, max(lr - 2, 0));
    r.fx = xi < 0 ? 0.0f : (xi > lr - 2 ? 1.0f : xs - xfl);
    r.wx0 = 1.0f - r.fx;
    return r;
}
__device__ __forceinline__ H2x2 lut_row_pair(const pbr_half* lut_, int lr, int y, int xb) {
    const H2* lut = reinterpret_cast<const H2*>(lut_);
    H2x2 lt;
    if (lr > 1) lt = *reinterpret_cast<const H2x2*>(reinterpret_cast<const char*>(lut) + (__umul24((uint32_t)y, (uint32_t)lr) + (uint32_t)xb) * 4u);   // 32-bit byte offsets: lr <= 16384 (host-checked)
    else lt.a = lt.b = lut[0];
    return lt;
}
__device__ __forceinline__ float lut_x_lerp(h16 a, h16 b, const LutX& x) { return __builtin_fmaf((float)b, x.fx, __builtin_fmaf((float)a, x.wx0, 0.0f)); }   // two v_fma_mix_f32, see fetch

// pbr_lut_fold_x: entry [y][rb] = the x-lerps of LUT row y's two channels at roughness byte rb, as two floats.  One thread per entry.
__global__ __launch_bounds__(256) void k_lut_fold_x(const pbr_half* __restrict__ lut, int lr, float* __restrict__ out) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;   // < lr * 256 <= 2^22
    const int y = (int)(t >> 8);
    if (y >= lr) return;
    const float roughness = (float)(t & 255u) * (1.0f / 255.0f);   // the pixel's decode of the C plane's byte
    const LutX x = lut_x_side(roughness, lr);
    const H2x2 lt = lut_row_pair(lut, lr, y, x.xb);
    reinterpret_cast<float2*>(out)[t] = make_float2(lut_x_lerp(lt.a.x, lt.b.x, x), lut_x_lerp(lt.a.y, lt.b.y, x));
}

// One pixel.  The kernel is bound by VALU ISSUE at 256 lights (SQ_ACTIVE_INST_VALU ~90 % of the launch), so the design
// constraints are instruction count and instruction class; measured issue costs on gfx950 at this kernel's occupancy of
// 5 waves per SIMD (tools/valu_rate3.hip -> profiles/r02_valu_rate3.txt, shader-clock cycles per wave-instruction per
// SIMD): v_fma_f32 2.6, v_mul/v_add 3.0, v_pk_{fma,mul,add}_f32 4.7, v_max/v_min 4.6, v_rcp/v_rsq 8.5; with one wave
// alone every plain op costs 7.5.  96 VGPRs (5 waves) is the measured optimum: 64 VGPRs (8 waves) spills heavily, 80 and
// 116 VGPRs time the same.  The pixel is shaded in phases that keep the live set small:
//   1. geometry: position, normal, view vector, roughness terms;
//   2. light loop: accumulates nine light-colour-weighted sums that do not depend on albedo/F0:
//        pl_c = Kdiff_c * S1_c + F0_c * spec_pix * S2_c + (1-F0_c) * spec_pix * S3_c
//        S1_c = sum col_c X (1-f5), S2_c = sum col_c X s, S3_c = sum col_c X s f5,   s = NdotL/(T A B)
//   3. material: re-reads the A/C planes (L2 hits) and folds the sums;
//   4. IBL: SH diffuse + split-sum specular from the padded env chain and the LUT.
template <bool STAGED_LISTS, int LSTRIDE, bool F32OUT, bool LUTFOLD>
__device__ __forceinline__ void shade_pixel(const ShadeParams& p, const float* llds, const uint32_t* lists, const uint32_t* mip_off,
                                            int n_lights, int q_safe, uint32_t px, uint32_t py, float4 row, float cvv_x, uint32_t col_list) {
    // 32-bit element index (host-checked: pitch * rows * 16 < 2^32): a uniform base + one 32-bit lane offset per access instead of
    // 64-bit address arithmetic for every plane
    const uint32_t gi = __umul24(py, p.pitch) + px;
    auto at = [](const auto* base, uint32_t byte_off) { return *reinterpret_cast<std::remove_reference_t<decltype(*base)>*>(reinterpret_cast<const char*>(base) + byte_off); };
    if (at(p.stencil, gi) == 0) return;   // stencil ref 0 < value (DeferredPipeline.h:176-181)
    const float inv255 = 1.0f / 255.0f;   // UNORM8 -> float

    // ---- phase 1: geometry (vs_main :91-121, screen triangle D3D12Device.cpp:167-176; uv from the GLOBAL pixel)
    // u, ndc_x, cvv.x and the cluster column depend on the pixel COLUMN only, v, cvv.y and the cluster row on the pixel ROW only: a
    // thread evaluates its column's once (k_deferred_shade: cvv_x, col_list), a block its rows' once per row (row = {InvView[1,4,7] *
    // cvv.y, the row's part of the list / cluster index}), the same expressions as ever — two IEEE divides, two floors, the clamps
    // and the index multiplies less per pixel
    V3 pos, view, n;
    float z_vs, roughness, depth_keep;
    {
        const uint32_t b = at(p.B, gi * 4u), c = at(p.C, gi * 4u);
        const float depth_ndc = at(p.depth, gi * 4u);
        // InvView * {cvv.x, cvv.y, Near}, in the order the contracted sum has always had: (I0 cvv.x + [I1 cvv.y]) + I2 Near, the
        // bracketed product rounded on its own (it is the row's)
        const V3 camera_vec = v3(__builtin_fmaf(p.InvView[2], p.Near, __builtin_fmaf(p.InvView[0], cvv_x, row.x)),
                                 __builtin_fmaf(p.InvView[5], p.Near, __builtin_fmaf(p.InvView[3], cvv_x, row.y)),
                                 __builtin_fmaf(p.InvView[8], p.Near, __builtin_fmaf(p.InvView[6], cvv_x, row.z)));
        roughness = (float)(c & 255u) * inv255;
        // (1 / 255 is NOT folded into the decode's 2 u - 1, unlike into the albedo's consumers below: the normal's last bit moves NdotH^2,
        //  which the GGX term t = NdotH^2 (a^4 - 1) + 1 amplifies ~1 / a^4 at a highlight.  Measured: one pixel of the 64 x 64 / 1024-light
        //  parity frame went from 2.4e-5 to 1.2e-4 of scale from the exact value, the fp32 restatement, which rounds u on its own, staying
        //  at 3.0e-5; and the compiler packs the two multiplies and the two fmas into one v_pk_mul + one v_pk_fma, so the fold saved nothing)
        n = normalize3(decode_octahedron((float)(b & 255u) * inv255, (float)((b >> 8) & 255u) * inv255));
        // ViewSpaceDepth :74-77, ReconstructWorldPosition :79-83.  Quick form (one v_rcp, <= 2 ulp): the position is continuous in
        // it; the cluster slice, which is not, re-evaluates the exact IEEE sequence wherever it could matter (below)
        z_vs = view_space_depth_quick(depth_ndc, p.Near, p.Far);
        depth_keep = depth_ndc;
        const V3 cam = v3(p.CameraPos[0], p.CameraPos[1], p.CameraPos[2]);
        const float zs = z_vs * p.inv_near;   // not an IEEE divide: the position is continuous in it (the slice index below is not, and keeps its divides)
        pos = v3(cam.x + camera_vec.x * zs, cam.y + camera_vec.y * zs, cam.z + camera_vec.z * zs);
        view = normalize3(cam - pos);
    }
    const float NdV = dot3(n, view);
    const float NdotV = fmaxf(NdV, 0.0f);

    // ---- phase 2: clustered point lights :159-186.  ClusterIndex(uv, z), clustered.hlsli:45-60;
    // logf (not the fast intrinsic): the result is truncated to the slice index.
    float s1x = 0.0f, s1y = 0.0f, s1z = 0.0f, s2x = 0.0f, s2y = 0.0f, s2z = 0.0f, s3x = 0.0f, s3y = 0.0f, s3z = 0.0f;
    // STAGED_LISTS: every staged list holds at least one pair (empty ones: two null lights), so the walk is a do-while with no
    // branch around it — with one, the compiler zeroes the 18 accumulator registers on both sides of every branch (36 moves per pixel)
#ifndef PBR_EXP_NOLOOP   // (PBR_EXP_*: compile-time switches of tools/isa_phase_count.py, which sizes the phases of this function)
    if (STAGED_LISTS || n_lights > 0) {
        float zc = fminf(fmaxf(z_vs, p.Near), p.Far);
        // Slice index = (int)(Z * logf(zc / Near) / log(Far / Near)), a discontinuous function of the depth: its value must be the
        // shader's / the oracle's to the bit, which takes two IEEE divides and a full-precision logf (~45 instructions).  A quick
        // estimate t = slice_k * v_log_f32(zc * inv_near) is within 5e-6 of that expression's real value (1-ulp log2 of
        // magnitude <= ~14, two rounded constants), and so is the exact sequence's own result: wherever t is further than 1e-4
        // from an integer both truncate alike.  Only waves with a lane inside that band (2e-4 of the pixels) run the sequence —
        // from the depth texel on: the quick view-space depth above (v_rcp) is within 2 ulp of the IEEE one, i.e. within 3e-7 of
        // its slice coordinate, far inside the band.
        const float t_quick = p.slice_k * __builtin_amdgcn_logf(zc * p.inv_near);
        const float t_frac = t_quick - floorf(t_quick);
        int sz = (int)t_quick;
#ifndef PBR_EXP_NOEXACT
        if (__any(!(t_frac > 1.0e-4f && t_frac < 1.0f - 1.0e-4f))) {
            zc = fminf(fmaxf(view_space_depth(depth_keep, p.Near, p.Far), p.Near), p.Far);
            sz = (int)((float)PBR_CLUSTER_Z * logf(zc / p.Near) / p.log_far_near);
        }
#endif
        sz = clampi(sz, 0, PBR_CLUSTER_Z - 1);
        // brdf() (brdf.hlsli:47-67) with D, G, the 4 NdotL NdotV denominator AND the attenuation under ONE reciprocal:
        //   D G / max(4 NdotL NdotV, 1e-4) = [a^2/pi * gV] * gl / (T * A),   a = roughness^2 (the shader's `a * a`),
        //   T  = max(t^2, 1e-6/pi), t = NdotH^2 (a^2 - 1) + 1,
        //   A  = NdotL(1-k)+k (>= 1/8: the shader's max(.,1e-6) never binds),
        //   gl = NdotL / max(4 NdotL NdotV, 1e-4) = min(1 / (4 NdotV), 1e4 NdotL)      (1 / max(a,b) = min(1/a, 1/b))
        //      = [1 / (4 NdotV)] * sat(NdotL * 4e4 NdotV): the saturation rides on a packed multiply (clamp modifier) where
        //      the min took two unpacked v_min, and the per-pixel factor 1 / (4 NdotV) moves out of the loop into spec_pix
        //      (where it cancels gV's NdotV: no division by NdotV is left),
        //   attenuation * NdotL = NdotL / Q;  with r = 1 / (Q T A):  1/Q = r T A,  so one v_rcp serves both; and T is
        //   carried as t^2 h2^2 (h2 = |L + V|^2), which removes the normalisation of H: 4 transcendentals per pair of lights.
        const float ra = roughness * roughness;
        const float a4m1 = ra * ra - 1.0f;
        const float k = (roughness + 1.0f) * (roughness + 1.0f) * 0.125f;
        const float one_k = 1.0f - k;
        const float c4 = 4.0e4f * NdotV;   // NdotV = 0: sat(0) = 0 here and spec_pix = 0 below, as gV = 0 makes the shader's term
        const float t_floor = EPSILON_F * INV_PI_F;
        // Instruction budget of the loop, from the measured issue costs (tools/valu_rate3.hip -> profiles/r02_valu_rate3.txt,
        // 5 waves per SIMD, cycles per wave-instruction per SIMD): v_pk_{fma,mul,add}_f32 4.7 (two lights per instruction),
        // plain v_fma 2.6 / v_mul 3.0, v_max / v_min 4.6, v_rsq / v_rcp 8.5.  Two lights per trip in the halves of packed
        // registers therefore buy ~1.2x per flop, not 2x; the SoA light planes put the same component of both lights into
        // an adjacent VGPR pair with no moves.  Per trip: 46 packed + 4 transcendental (+ 2 / 4 v_max on the slow paths); the loop's compare and pointer step come once per WALK_TRIPS trips.
        // the nine packed sums start at zero: ONE v_pk_mov_b32 per register pair (the compiler writes two v_mov_b32 per pair)
        f2 a1x = zero2(), a1y = zero2(), a1z = zero2(), a2x = zero2(), a2y = zero2(), a2z = zero2(), a3x = zero2(), a3y = zero2(), a3z = zero2();
        const float att_c0 = llds[6 * LSTRIDE], att_c1 = llds[7 * LSTRIDE], att_c2 = llds[8 * LSTRIDE];   // light 0's polynomial (ATT: everyone's)
        auto light2 = [&](auto q_safe, auto t_safe, const lds_cf* la, const lds_cf* lb, auto att_uniform) {
            constexpr bool QSAFE = decltype(q_safe)::value, TSAFE = decltype(t_safe)::value, ATT = decltype(att_uniform)::value;
            auto comp = [&](int c) { return f2{la[c * LSTRIDE], lb[c * LSTRIDE]}; };
            const f2 dx = comp(0) - f2s(pos.x), dy = comp(1) - f2s(pos.y), dz = comp(2) - f2s(pos.z);
            const f2 d2 = dx * dx + dy * dy + dz * dz;
            const f2 invd = rsq2(d2);
            const f2 dn = dx * n.x + dy * n.y + dz * n.z;
            const f2 NdotL = mul2_sat(dn, invd);   // max(N.L, 0)
            // |L + V|^2 is summed from the components of L + V, NOT taken as 2 + 2 L.V: at grazing incidence (L ~ -V,
            // |L + V|^2 ~ 1e-2) the shortcut cancels and its 1e-7 error becomes 1e-5 of N.H, which a GGX highlight at
            // roughness 0.2 (t ~ 2e-3) multiplies by 4 / t: several per cent of D (measured against the oracle on a 4K
            // band: 3 pixels of 122 880).  One packed instruction more than the shortcut.
            const f2 wx = dx * invd + f2s(view.x), wy = dy * invd + f2s(view.y), wz = dz * invd + f2s(view.z);
            // (the 1e-15 keeps h2 > 0 when L = -V exactly, so that the shared reciprocal below stays finite; it is
            //  ten orders of magnitude below any |L + V|^2 that contributes light)
            const f2 h2 = wx * wx + (wy * wy + (wz * wz + f2s(1.0e-15f)));
            // GGX without normalising H at all: with nw = N.(L + V) and h2 = |L + V|^2, N.H^2 = nw^2 / h2 and
            //   t = N.H^2 (a^2 - 1) + 1 = tn / h2,  tn = nw^2 (a^2 - 1) + h2,   so  1 / t^2 = h2^2 / tn^2
            // which joins the one reciprocal of the trip: no v_rsq for H.  nw < 0 (the shader clamps N.H to 0 there)
            // needs no case: N.L > 0 then forces N.V < 0, which zeroes the specular term through spec_pix.
            const f2 nw = dn * invd + f2s(NdV);
            const f2 tn = (nw * nw) * a4m1 + h2;
            const f2 h4 = h2 * h2;
            // TSAFE: every active lane of the wave has a^2 >= 6e-4, hence t >= a^2 - 6e-8 > sqrt(1e-6 / pi) = 5.64e-4 and the
            // shader's max(pi t^2, 1e-6) never binds (decided per wave before the walk)
            f2 Tn = tn * tn;                                 // t^2 h2^2
            if constexpr (!TSAFE) Tn = max2(Tn, h4 * t_floor);
            const f2 A = NdotL * one_k + f2s(k);
            // attenuation(): max(C0 + C1 d + C2 d^2, 1e-6).  QSAFE: every staged light has C0 >= 1e-6 and C1, C2 >= 0,
            // so the floor never binds (checked once per block while the table is staged)
            f2 Q;
            // C0 + C1 d + C2 d^2 with d = d2 / sqrt(d2) never formed: d2 (C1 invd + C2) + C0 — two fused operations
            if constexpr (ATT) Q = d2 * (invd * f2s(att_c1) + f2s(att_c2)) + f2s(att_c0);   // the scene's one polynomial (the null light takes it too: its colour is 0 and Q stays finite)
            else Q = d2 * (invd * comp(7) + comp(8)) + comp(6);
            if constexpr (!QSAFE) Q = max2(Q, f2s(EPSILON_F));
            const f2 TA = Tn * A;
            const f2 r = rcp2(Q * TA);                       // 1 / (Q A t^2 h2^2)
            const f2 q = NdotL * r;
            const f2 X = q * TA;                             // attenuation * NdotL = NdotL / Q
            const f2 gs = mul2_sat(NdotL, f2s(c4));          // gl * 4 NdotV
            // fresnel on NdotL (Q3).  The shader's max(1-NdotL, 1e-6) only matters within 1e-6 of NdotL = 1, where it
            // changes f5 by < 1e-30: dropped.
            const f2 fm = f2s(1.0f) - NdotL;
            const f2 fm2 = fm * fm;
            const f2 f5 = fm2 * fm2 * fm;
            const f2 w2 = (q * gs) * h4;                     // X * gl / (t^2 A) * 4 NdotV
            const f2 w1 = X - X * f5;                        // X * (1 - f5)
            const f2 w3 = w2 * f5;
            const f2 cr = comp(3), cg = comp(4), cb = comp(5);
            a1x += cr * w1; a1y += cg * w1; a1z += cb * w1;
            a2x += cr * w2; a2y += cg * w2; a2z += cb * w2;
            a3x += cr * w3; a3y += cg * w3; a3z += cb * w3;
        };
        const lds_cf* const ltab = (const lds_cf*)llds;      // the staged light planes, as an LDS (address space 3) pointer
        if (STAGED_LISTS) {
            // (col_list, row.w: the column's and the row's part of the list's dword offset)
            const uint32_t* my = lists + (__umul24((uint32_t)sz, LIST_STRIDE) + col_list + __float_as_uint(row.w));
            // staged lists are padded to a multiple of 2 WALK_TRIPS entries with the null light (black, far away): the walk takes WALK_TRIPS trips
            // per pointer step and compare, and the null light adds +0 to sums that start at +0: every sum keeps its bits.  An entry is
            // the LDS BYTE ADDRESS of the light's first plane (table base + 4 * index), a dword of its own: packed two to a dword
            // the unpacking mask + shift were two more VALU issues per trip
            const int nl = my[0];
            const bool t_ok = __all(ra * ra >= 6.0e-4f) != 0;
            auto walk = [&](auto qs, auto ts, auto au) {
                int i = 0;
                do {   // nl >= 2 WALK_TRIPS, a multiple of it.  One 8-byte LDS read = the two addresses of a trip, each in its own register; the later trips' ride on the DS offset field
#pragma unroll
                    for (int k = 0; k < WALK_TRIPS; k++) {
                        const uint2 pair = *reinterpret_cast<const uint2*>(my + 2 + i + 2 * k);   // i even -> 8-byte aligned
                        light2(qs, ts, (const lds_cf*)(uintptr_t)pair.x, (const lds_cf*)(uintptr_t)pair.y, au);
                    }
                    i += 2 * WALK_TRIPS;
                } while (i < nl);
                // (reading the NEXT trip's two entries one trip ahead was measured in round 4: two more live registers push the
                //  kernel's scratch from 12 to 24 bytes per lane at its 96-VGPR budget, in-frame 0.3356 -> 0.3470 ms; removed —
                //  profiles/r04_d_ab_shade_prefetch.txt)
            };
            if (q_safe & 1) {
                if (t_ok) { if (q_safe & 2) walk(std::true_type{}, std::true_type{}, std::true_type{}); else walk(std::true_type{}, std::true_type{}, std::false_type{}); }
                else if (q_safe & 2) walk(std::true_type{}, std::false_type{}, std::true_type{});   // a rough-enough wave is a property of the PIXELS, one polynomial of the SCENE: independent
                else walk(std::true_type{}, std::false_type{}, std::false_type{});
            } else walk(std::false_type{}, std::false_type{}, std::false_type{});
        } else {
            const pbr_cluster* cl = p.clusters + ((uint32_t)sz + col_list + __float_as_uint(row.w));
            const int nl = min(max(cl->NumLights, 0), PBR_MAX_LIGHTS_PER_CLUSTER);
            auto idx = [&](int q) { return q < nl ? min(max(cl->LightIndex[q], 0), n_lights - 1) : n_lights; };   // n_lights = the null light
            for (int i = 0; i < nl; i += 2) light2(std::false_type{}, std::false_type{}, ltab + idx(i), ltab + idx(i + 1), std::false_type{});
        }
        s1x = a1x.x + a1x.y; s1y = a1y.x + a1y.y; s1z = a1z.x + a1z.y;
        s2x = a2x.x + a2x.y; s2y = a2y.x + a2y.y; s2z = a2z.x + a2z.y;
        s3x = a3x.x + a3x.y; s3y = a3y.x + a3y.y; s3z = a3z.x + a3z.y;
    }
#endif

    // ---- phase 3: material terms (planes A and C re-read: L2 hits, keeps them out of the loop's registers)
    const uint32_t a = at(p.A, gi * 4u);
    // the albedo bytes are never scaled on their own: 1 / 255 rides on the operation that consumes them
    const float metal_b = (float)((at(p.C, gi * 4u) >> 8) & 255u), metallic = metal_b * inv255;
    const V3 albedo_b = v3((float)(a & 255u), (float)((a >> 8) & 255u), (float)((a >> 16) & 255u));
    const float emission = (float)(a >> 24) * (inv255 * inv255);   // emission / 255: albedo_b * emission = albedo * emission
    const V3 F0 = v3(__builtin_fmaf(metallic, __builtin_fmaf(albedo_b.x, inv255, -0.04f), 0.04f),
                     __builtin_fmaf(metallic, __builtin_fmaf(albedo_b.y, inv255, -0.04f), 0.04f),
                     __builtin_fmaf(metallic, __builtin_fmaf(albedo_b.z, inv255, -0.04f), 0.04f));
    V3 out;
    {
        const float ra = roughness * roughness;
        const float k = (roughness + 1.0f) * (roughness + 1.0f) * 0.125f;
        // a^2 / pi * gV / (4 NdotV), gV = NdotV / max(NdotV (1-k) + k, 1e-6): the light sums S2, S3 carry gl * 4 NdotV
        const float spec_pix = NdotV > 0.0f ? ra * ra * (0.25f * INV_PI_F) * rcp(fmaxf(NdotV * (1.0f - k) + k, EPSILON_F)) : 0.0f;
        // Kd*albedo/pi = (1-F0)(1-m) albedo/pi * (1-f5); (1-m)/pi/255 = (255 - byte) / (255^2 pi): the difference of the bytes is exact,
        // so a metal (byte 255) has kd = 0 as the shader's 1 - metallic has, and a near-metal the relative accuracy of every other
        // pixel.  (As fma(byte, -k1, k0) the two rounded constants left -7.1e-11 at byte 255 — a negative half subnormal in the target
        // — and 255 times the relative error at byte 254.)  Its product with the albedo byte serves the light fold and the SH term
        const float kd = (255.0f - metal_b) * (inv255 * inv255 * INV_PI_F);
        const V3 kda = v3(kd * albedo_b.x, kd * albedo_b.y, kd * albedo_b.z);
        out.x = (1.0f - F0.x) * (kda.x * s1x + spec_pix * s3x) + F0.x * spec_pix * s2x;
        out.y = (1.0f - F0.y) * (kda.y * s1y + spec_pix * s3y) + F0.y * spec_pix * s2y;
        out.z = (1.0f - F0.z) * (kda.z * s1z + spec_pix * s3z) + F0.z * spec_pix * s2z;
        // emission (Q1: the directional light of :144-156 is computed by the reference but never added)
        out = out + albedo_b * emission;

        // ---- phase 4a: EnvironmentDiffuse :23-54
#ifndef PBR_EXP_NOSH
        const float bx = n.x * n.y, by = n.y * n.z, bz = n.z * n.z, bw = n.z * n.x;
        const float cc = n.x * n.x - n.y * n.y;
        const pbr_sh_pack& s = p.sh;
        const float ir = (s.sha_r[0] * n.x + s.sha_r[1] * n.y + s.sha_r[2] * n.z + s.sha_r[3]) +
                         ((s.shb_r[0] * bx + s.shb_r[1] * by + s.shb_r[2] * bz + s.shb_r[3] * bw) + s.shc[0] * cc);
        const float ig = (s.sha_g[0] * n.x + s.sha_g[1] * n.y + s.sha_g[2] * n.z + s.sha_g[3]) +
                         ((s.shb_g[0] * bx + s.shb_g[1] * by + s.shb_g[2] * bz + s.shb_g[3] * bw) + s.shc[1] * cc);
        const float ib = (s.sha_b[0] * n.x + s.sha_b[1] * n.y + s.sha_b[2] * n.z + s.sha_b[3]) +
                         ((s.shb_b[0] * bx + s.shb_b[1] * by + s.shb_b[2] * bz + s.shb_b[3] * bw) + s.shc[2] * cc);
        out.x += kda.x * ir;
        out.y += kda.y * ig;
        out.z += kda.z * ib;
#endif
    }

    // ---- phase 4b: EnvironmentSpecular :56-70 — padded env chain: each bilinear row is one 16-byte pair
#ifndef PBR_EXP_NOIBL
    {
#ifndef PBR_EXP_NOENV
        const V3 R = normalize3(n * (2.0f * NdV) - view);
        float lod = roughness * (float)PBR_ENV_MIPS;   // Q4: roughness*5 on a 5-mip chain
        lod = snap8(fminf(fmaxf(lod, 0.0f), (float)(p.env_mips - 1)));   // 8-bit LOD fraction
        const float fl = floorf(lod);
        const uint32_t l0 = (uint32_t)fl, l1 = min(l0 + 1, p.env_mips - 1);
        const float env_f = lod - fl;
        // face + uv of R (D3D cube addressing).  v_rcp instead of an IEEE divide: u,v only feed a continuous filter
        uint32_t face;
        float cu, cv;
        {
            // the cube-map coordinate instructions (v_cubeid / v_cubesc / v_cubetc / v_cubema: D3D face order and (sc, tc)
            // table; ma = 2 x the signed major axis): 4 instructions for the three-way compare-and-select.  On an exact tie
            // of two |components| they pick z, then y, then x where the shader's HLSL picks x, then y, then z — the same
            // point on the shared edge of two faces, which the seamless footprints filter alike.
            const float ma = 0.5f * fabsf(__builtin_amdgcn_cubema(R.x, R.y, R.z));
            const float sc = __builtin_amdgcn_cubesc(R.x, R.y, R.z), tc = __builtin_amdgcn_cubetc(R.x, R.y, R.z);
            face = (uint32_t)__builtin_amdgcn_cubeid(R.x, R.y, R.z);
            const float inv = rcp(ma);
            cu = (sc * inv + 1.0f) * 0.5f;
            cv = (tc * inv + 1.0f) * 0.5f;
        }
        // One trilinear sample = eight texels x eight weights.  The shader's nested lerps (x, then y, then level) cost 2 products per
        // lerp and channel (47 instructions for the three channels); as a weighted sum — weights (1-fx | fx)(1-fy | fy)(1-f | f),
        // 10 multiplies once — each texel is ONE v_fma_mix_f32 per channel (34 instructions).  The two forms differ by rounding
        // only (~3 ulp of fp32 on a convex combination of fp16 texels).
        struct Foot { H4x2 r0, r1; float w00, w10, w01, w11; };
        auto foot = [&](uint32_t l, uint32_t mip_off, float wl) {
            const int s = (int)(p.env_size >> l), sq = s + 1;
            // u in [0,1] -> texel coordinate in [-0.5, s-0.5]: no NaN / range guard needed here; x.8 fixed-point snap
            const float fxp = snap8(cu * (float)s) - 0.5f, fyp = snap8(cv * (float)s) - 0.5f;
            const float flx = floorf(fxp), fly = floorf(fyp);
            const float fx = fxp - flx, fy = fyp - fly;
            // footprint layout: the four texels of this tap are 32 contiguous bytes.  24-bit multiplies (every factor < 2^24;
            // v_mul_lo_u32 / v_mad_u64_u32 are multi-pass instructions) and a 32-bit byte offset from the chain's base
            // (host-checked: the padded chain is smaller than 4 GiB)
            const uint32_t o = __umul24(__umul24(face, (uint32_t)sq) + (uint32_t)((int)fly + 1), (uint32_t)sq) + (uint32_t)((int)flx + 1);
            const char* q = reinterpret_cast<const char*>(p.env) + (mip_off + o * 4u) * 8u;
            Foot f;
            f.r0 = *reinterpret_cast<const H4x2*>(q);
            f.r1 = *reinterpret_cast<const H4x2*>(q + 16);
            const float wy1 = fy * wl, wy0 = wl - wy1;         // (1 - fy) wl, fy wl
            f.w10 = fx * wy0; f.w00 = wy0 - f.w10;             // (1 - fx)(1 - fy) wl, fx (1 - fy) wl
            f.w11 = fx * wy1; f.w01 = wy1 - f.w11;
            return f;
        };
        const Foot fa = foot(l0, mip_off[l0], 1.0f - env_f);   // per-lane index: the table sits in LDS (an SGPR array would spill to scratch)
        const Foot fb = foot(l1, mip_off[l1], env_f);
        auto chan = [&](h16 a00, h16 a10, h16 a01, h16 a11, h16 b00, h16 b10, h16 b01, h16 b11) {
            float r = __builtin_fmaf((float)a00, fa.w00, 0.0f);   // fma(x, w, 0): the first product as v_fma_mix_f32 too (no separate v_cvt)
            r = __builtin_fmaf((float)a10, fa.w10, r);
            r = __builtin_fmaf((float)a01, fa.w01, r);
            r = __builtin_fmaf((float)a11, fa.w11, r);
            r = __builtin_fmaf((float)b00, fb.w00, r);
            r = __builtin_fmaf((float)b10, fb.w10, r);
            r = __builtin_fmaf((float)b01, fb.w01, r);
            return __builtin_fmaf((float)b11, fb.w11, r);
        };
        const V3 envc = v3(chan(fa.r0.a.x, fa.r0.b.x, fa.r1.a.x, fa.r1.b.x, fb.r0.a.x, fb.r0.b.x, fb.r1.a.x, fb.r1.b.x),
                           chan(fa.r0.a.y, fa.r0.b.y, fa.r1.a.y, fa.r1.b.y, fb.r0.a.y, fb.r0.b.y, fb.r1.a.y, fb.r1.b.y),
                           chan(fa.r0.a.z, fa.r0.b.z, fa.r1.a.z, fa.r1.b.z, fb.r0.a.z, fb.r0.b.z, fb.r1.a.z, fb.r1.b.z));
#else
        const V3 envc = v3(0.5f, 0.5f, 0.5f);
#endif
#ifndef PBR_EXP_NOLUT
        // LUT bilinear with clamp addressing (Q5): one 8-byte pair per row (the x side: lut_x_side above).  N.V is clamped to [0, 1]:
        // no NaN / range guard; x.8 fixed-point snap as in pbr_device.hpp::bilinear_coord.
        const int lr = (int)p.lut_res;
        const float ys = snap8(NdotV * (float)lr) - 0.5f;
        const float yfl = floorf(ys);
        const int yi = (int)yfl;
        const int y0 = clampi(yi, 0, lr - 1), y1 = clampi(yi + 1, 0, lr - 1);
        const float fy = ys - yfl, wy0 = 1.0f - fy;
        float la, lb;
        if constexpr (LUTFOLD) {
            // the x-lerps of both rows come ready from the folded table (entry [row][roughness byte], 8 bytes: the same two gathers);
            // the y-lerp in the association the sampled form's contraction has: fma(X0, wy0, X1 * fy)
            // the entry's byte offset in its row, 8 x the roughness byte, from the float in hand (byte / 255 rounded: 2040 x it is within
            // 3e-4 of 8 x byte, so + 0.5 truncates to it): two instructions, like (c & 255) * 8 on the C plane's re-read, which timed the same
            const uint32_t rb8 = (uint32_t)__builtin_fmaf(roughness, 2040.0f, 0.5f);
            const char* ft = reinterpret_cast<const char*>(p.lut_fold);
            const float2 f0 = *reinterpret_cast<const float2*>(ft + (((uint32_t)y0 << 11) | rb8));   // 32-bit byte offsets: lr <= 16384
            const float2 f1 = *reinterpret_cast<const float2*>(ft + (((uint32_t)y1 << 11) | rb8));
            la = __builtin_fmaf(f0.x, wy0, f1.x * fy);
            lb = __builtin_fmaf(f0.y, wy0, f1.y * fy);
        } else {
            const LutX lx = lut_x_side(roughness, lr);
            const H2x2 lt0 = lut_row_pair(p.lut, lr, y0, lx.xb), lt1 = lut_row_pair(p.lut, lr, y1, lx.xb);
            la = lut_x_lerp(lt0.a.x, lt0.b.x, lx) * wy0 + lut_x_lerp(lt1.a.x, lt1.b.x, lx) * fy;
            lb = lut_x_lerp(lt0.a.y, lt0.b.y, lx) * wy0 + lut_x_lerp(lt1.a.y, lt1.b.y, lx) * fy;
        }
#else
        const float la = 0.5f, lb = 0.25f;
#endif
        out.x += envc.x * (F0.x * la + lb);
        out.y += envc.y * (F0.y * la + lb);
        out.z += envc.z * (F0.z * la + lb);
    }
#endif
    const uint32_t ho = __umul24(py, p.hdr_pitch) + px;
    if (F32OUT) *reinterpret_cast<float4*>(reinterpret_cast<char*>(p.hdr_f32) + ho * 16u) = make_float4(out.x, out.y, out.z, 1.0f);
    else store_h4(reinterpret_cast<pbr_half*>(reinterpret_cast<char*>(p.hdr) + ho * 8u), f4(out.x, out.y, out.z, 1.0f));
}

#ifdef PBR_SHADE_TIMING   // experiment build only (tools/shade_timeline.py): 100 MHz wall-clock stamps of every block
__device__ unsigned long long g_shade_item_stamp[4 * 160000];    // per block: start, tables staged, end (last wave), (rows << 48 | block)
extern "C" int pbr_debug_shade_stamps(unsigned long long* blocks, int n_blocks, unsigned long long* items, int n_items) {
    (void)blocks; (void)n_blocks;
    return (int)hipMemcpyFromSymbol(items, HIP_SYMBOL(g_shade_item_stamp), sizeof(unsigned long long) * 4 * n_items);
}
extern "C" int pbr_debug_shade_stamps_reset() {
    void* i = nullptr;
    int e = (int)hipGetSymbolAddress(&i, HIP_SYMBOL(g_shade_item_stamp));
    if (e == 0) e = (int)hipMemset(i, 0, sizeof(g_shade_item_stamp));
    return e;
}
#define SHADE_ISTAMP(it, i, v) do { if (threadIdx.x == 0 && (it) < 160000u) g_shade_item_stamp[(it) * 4 + (i)] = (v); } while (0)
// end stamp: the LAST wave of the block to get there (the array is zeroed before the launch)
#define SHADE_ISTAMP_MAX(it, i, v) do { if ((threadIdx.x & 63) == 0 && (it) < 160000u) atomicMax(&g_shade_item_stamp[(it) * 4 + (i)], (v)); } while (0)
#define SHADE_NOW() wall_clock64()
#else
#define SHADE_ISTAMP(it, i, v) do {} while (0)
#define SHADE_ISTAMP_MAX(it, i, v) do {} while (0)
#define SHADE_NOW() 0ull
#endif

// ---- what the shade kernels' prologues share -----------------------------------------------------------------------------------------
// The block's pixels, as the locals both kernels name: columns [bx0, min(bx0 + SHADE_BLOCK, x_end)), rows [y_begin, y_end) of the tile.
// block -> rectangle -> (column block, row block); wave-uniform scalar arithmetic.  Two-zone schedule: the first nb_big block rows walk
// rows_big rows each, the rest rows_small — the short blocks are dispatched last and fill the tail of the launch (a 4K frame is only ~3.2
// waves of resident blocks).  A macro: as a function returning the four it reordered every shade kernel.
#define SHADE_BLOCK_SPAN(rc)                                                                                                             \
    uint32_t r = 0;                                                                                                                      \
    while (r + 1 < rc.n && blockIdx.x >= rc.first[r + 1]) r++;                                                                           \
    const uint32_t lb = blockIdx.x - rc.first[r];                                                                                        \
    const uint32_t bx0 = rc.x0[r] + (lb % rc.cols[r]) * SHADE_BLOCK, x_end = rc.x0[r] + rc.w[r];                                         \
    const uint32_t by = lb / rc.cols[r], nb_big = rc.nb_big[r], rows_big = rc.rows_big, rows_small = rc.rows_small;                      \
    const uint32_t y_begin = rc.y0[r] + (by < nb_big ? by * rows_big : nb_big * rows_big + (by - nb_big) * rows_small);                  \
    const uint32_t y_end = min(y_begin + (by < nb_big ? rows_big : rows_small), rc.y0[r] + rc.h[r])

// The dynamic LDS of a block, as the locals both kernels name: 9 planes * LSTRIDE floats of light data (llds), then (staged lists)
// max_clusters * 136 B of light lists (lists, 8-byte aligned); lds_base: the planes' LDS byte address, < 64 KiB: the whole light table
// (<= 9 x 1025 floats) stays addressable in 16 bits
#define SHADE_LDS_CARVE(LSTRIDE)                                                                          \
    extern __shared__ float4 lds_raw[];                                                                   \
    float* const llds = reinterpret_cast<float*>(lds_raw);                                                \
    uint32_t* const lists = reinterpret_cast<uint32_t*>(llds + ((LIGHT_PLANES * LSTRIDE + 1) & ~1));      \
    const uint32_t lds_base = (uint32_t)(uintptr_t)(lds_cf*)llds

// The column term of global pixel column gx and the row term of global pixel row gy of a full_w x full_h frame (vs_main :91-95,
// ClusterIndex clustered.hlsli:46-47; uv from the GLOBAL pixel): half the NDC coordinate (times the near plane's size: cvv) and the cluster
// column / row — IEEE divide, floor, clamp.  Monotone in the pixel coordinate, so a rectangle's corners bound its cluster tiles.
// k_shade_geometry_tables stores exactly these; the tabled kernel reads them back, the computed one evaluates them: bit-exact by construction.
struct alignas(8) AxisTerm { float half_ndc; int cluster; };   // (also an entry of the geometry tables)
__device__ __forceinline__ AxisTerm shade_column_term(uint32_t gx, uint32_t full_w) {
    const float u = ((float)gx + 0.5f) / (float)full_w;
    const float ndc_x = 2.0f * u - 1.0f;
    return AxisTerm{ndc_x * 0.5f, clampi((int)floorf(u * (float)PBR_CLUSTER_X), 0, PBR_CLUSTER_X - 1)};
}
__device__ __forceinline__ AxisTerm shade_row_term(uint32_t gy, uint32_t full_h) {
    const float v = ((float)gy + 0.5f) / (float)full_h;
    const float ndc_y = 1.0f - 2.0f * v;
    return AxisTerm{ndc_y * 0.5f, clampi((int)floorf((1.0f - v) * (float)PBR_CLUSTER_Y), 0, PBR_CLUSTER_Y - 1)};
}
// A row's s_row entry and a column's col_list from their terms: InvView's column 1 times cvv.y, and the row's / the column's part of the
// index of the pixel's list (staged: dwords from `lists`, relative to the block's first tile) or cluster (global: clusters from p.clusters)
template <bool STAGED_LISTS>
__device__ __forceinline__ float4 shade_row_entry(const ShadeParams& p, AxisTerm row, int tile_y0, int tiles_x) {
    const float cvv_y = row.half_ndc * p.near_height;
    const uint32_t row_list = STAGED_LISTS ? (uint32_t)((row.cluster - tile_y0) * tiles_x * (PBR_CLUSTER_Z * LIST_STRIDE)) : (uint32_t)(row.cluster * (PBR_CLUSTER_X * PBR_CLUSTER_Z));
    return make_float4(p.InvView[1] * cvv_y, p.InvView[4] * cvv_y, p.InvView[7] * cvv_y, __uint_as_float(row_list));
}
template <bool STAGED_LISTS>
__device__ __forceinline__ uint32_t shade_col_list(int cluster, int tile_x0) {
    return STAGED_LISTS ? (uint32_t)((cluster - tile_x0) * (PBR_CLUSTER_Z * LIST_STRIDE)) : (uint32_t)(cluster * PBR_CLUSTER_Z);
}

// The block's rows, once its tables are staged, over the locals both kernels name; ...: shade_pixel's template arguments.  The stamps are no-ops
// in the product build, whose threads right of x_end leave the kernel at once; in the timing build k_deferred_shade's "tables staged" stamp
// follows the thread's column term.  A macro: as a function, or reading the span's members at the uses, it cost the staged kernels two more
// s_waitcnt in the row loop and the fp32 probe 8 bytes of scratch.
#define SHADE_ROW_LOOP(...)                                                                                                         \
    do {                                                                                                                            \
        (void)t_start;                                                                                                              \
        SHADE_ISTAMP(blockIdx.x, 0, t_start);                                                                                       \
        SHADE_ISTAMP(blockIdx.x, 1, SHADE_NOW());                                                                                   \
        SHADE_ISTAMP(blockIdx.x, 3, ((unsigned long long)(y_end - y_begin) << 48) | blockIdx.x);                                    \
        if (px < x_end)                                                                                                             \
            for (uint32_t py = y_begin; py < y_end; py++)                                                                           \
                shade_pixel<__VA_ARGS__>(p, llds, lists, s_mip_off, n_lights, q_safe, px, py, s_row[py - y_begin], cvv_x, col_list); \
        SHADE_ISTAMP_MAX(blockIdx.x, 2, SHADE_NOW());                                                                               \
    } while (0)

// grid: rc.first[rc.n] blocks of 256 threads, dispatched in index order (the hardware's dispatcher is the work queue: a software queue
// of persistent blocks was built and measured in round 6 and lost to it at every size — EXPERIMENTS.md).
#ifndef SHADE_MIN_WAVES
#define SHADE_MIN_WAVES 5   // 96 VGPRs; 2 dwords of scratch per lane are spilled OUTSIDE the light loop.  Best of 4..8 measured (tools/probe_shade.py)
#endif
// (an exact register budget cannot be asked for: `amdgpu_num_vgpr(104)` is ignored beside the waves-per-EU bound on gfx950 — round 6, EXPERIMENTS.md)
// Multi-view shade (pbr_deferred_shade_views): k_deferred_shade<.., ShadeViews>, grid (blocks of ONE view, views).  p_ holds what the views
// share (size, LUT, env chain, SH pack); a view's camera, planes, clusters, lights and target come from its ShadeView.
struct ShadeView {
    float InvView[9], CameraPos[3];
    float Near, Far, near_width, near_height, log_far_near, inv_near, slice_k;
    const uint32_t* A;
    const uint32_t* B;
    const uint32_t* C;
    const float* depth;
    const uint8_t* stencil;
    const pbr_cluster* clusters;
    const pbr_light* lights;
    pbr_half* hdr;
    uint32_t pitch, hdr_pitch;
    int n_lights;
};
struct ShadeViews { ShadeView v[PBR_MAX_VIEWS]; };
static_assert(sizeof(ShadeParams) + sizeof(ShadeViews) + sizeof(ShadeRects) + 16 <= 4096 - 256, "k_deferred_shade<.., ShadeViews>: kernel arguments over 4 KiB");

// LUTFOLD: the split-sum LUT is read from its x-folded table (p.lut_fold, pbr_lut_fold_x) — the same bits with ~30 instructions less per pixel.
template <bool STAGED_LISTS, int LSTRIDE, bool F32OUT, class VS = NoViews, bool LUTFOLD = false>
__global__ __launch_bounds__(SHADE_BLOCK, SHADE_MIN_WAVES) void k_deferred_shade(ShadeParams p_, int n_lights_, int max_clusters, ShadeRects rc, VS vs) {
    constexpr bool MV = !std::is_same_v<VS, NoViews>;   // VS = ShadeViews: view blockIdx.y of vs; NoViews (empty): the single-view kernel
    ShadeParams q;                                      // MV: p_ with the view's fields
    int n_views_lights = 0;
    if constexpr (MV) {
        const ShadeView& v = vs.v[blockIdx.y];
        q = p_;
        for (int i = 0; i < 9; i++) q.InvView[i] = v.InvView[i];
        for (int i = 0; i < 3; i++) q.CameraPos[i] = v.CameraPos[i];
        q.Near = v.Near; q.Far = v.Far; q.near_width = v.near_width; q.near_height = v.near_height;
        q.log_far_near = v.log_far_near; q.inv_near = v.inv_near; q.slice_k = v.slice_k;
        q.A = v.A; q.B = v.B; q.C = v.C; q.depth = v.depth; q.stencil = v.stencil; q.pitch = v.pitch;
        q.clusters = v.clusters; q.lights = v.lights; q.hdr = v.hdr; q.hdr_pitch = v.hdr_pitch;
        n_views_lights = v.n_lights;
    }
    const ShadeParams& p = MV ? q : p_;
    const int n_lights = MV ? n_views_lights : n_lights_;
    __shared__ uint32_t s_mip_off[16];
    const unsigned long long t_start = SHADE_NOW();
    if (threadIdx.x < 16) s_mip_off[threadIdx.x] = p_.env_mip_off[threadIdx.x];   // (p_: a per-lane index into the local copy would live in scratch)
    SHADE_LDS_CARVE(LSTRIDE);
    int my_safe = 1, my_same = 1;
    const float att0 = n_lights > 0 ? p.lights[0].C0 : 1.0f, att1 = n_lights > 0 ? p.lights[0].C1 : 0.0f, att2 = n_lights > 0 ? p.lights[0].C2 : 0.0f;
    if (threadIdx.x == 0) {   // the null light: pads odd lists; black, so its pair lane contributes exactly 0
        llds[0 * LSTRIDE + n_lights] = 1.0e15f; llds[1 * LSTRIDE + n_lights] = 1.0e15f; llds[2 * LSTRIDE + n_lights] = 1.0e15f;
        llds[3 * LSTRIDE + n_lights] = 0.0f; llds[4 * LSTRIDE + n_lights] = 0.0f; llds[5 * LSTRIDE + n_lights] = 0.0f;
        llds[6 * LSTRIDE + n_lights] = 1.0f; llds[7 * LSTRIDE + n_lights] = 0.0f; llds[8 * LSTRIDE + n_lights] = 0.0f;
    }
    for (int i = threadIdx.x; i < n_lights; i += SHADE_BLOCK) {
        const pbr_light l = p.lights[i];
        my_safe &= (l.C0 >= EPSILON_F) & (l.C1 >= 0.0f) & (l.C2 >= 0.0f);
        my_same &= (l.C0 == att0) & (l.C1 == att1) & (l.C2 == att2);
        llds[0 * LSTRIDE + i] = l.Position[0];
        llds[1 * LSTRIDE + i] = l.Position[1];
        llds[2 * LSTRIDE + i] = l.Position[2];
        llds[3 * LSTRIDE + i] = l.Color[0] * l.Intensity;
        llds[4 * LSTRIDE + i] = l.Color[1] * l.Intensity;
        llds[5 * LSTRIDE + i] = l.Color[2] * l.Intensity;
        llds[6 * LSTRIDE + i] = l.C0;
        llds[7 * LSTRIDE + i] = l.C1;
        llds[8 * LSTRIDE + i] = l.C2;
    }
    SHADE_BLOCK_SPAN(rc);
    int tile_x0 = 0, tile_y0 = 0, tiles_x = 1;
    if (STAGED_LISTS) {
        // cluster (x,y) tiles the block's pixel rectangle can fall into: the cluster column / row of its corners
        const uint32_t bx1 = min(bx0 + SHADE_BLOCK, x_end) - 1;
        auto tx = [&](uint32_t x) { return shade_column_term(p.x0 + x, p.full_w).cluster; };
        auto ty = [&](uint32_t y) { return shade_row_term(p.y0 + y, p.full_h).cluster; };
        tile_x0 = tx(bx0);
        const int tile_x1 = tx(bx1);
        const int ty_a = ty(y_begin), ty_b = ty(y_end - 1);
        tile_y0 = min(ty_a, ty_b);
        const int tile_y1 = max(ty_a, ty_b);
        tiles_x = tile_x1 - tile_x0 + 1;
        const int n_cl = min(tiles_x * (tile_y1 - tile_y0 + 1) * PBR_CLUSTER_Z, max_clusters);   // host sized the LDS for the worst case
        {
            static_assert(PBR_CLUSTER_Z == 8 && PBR_MAX_LIGHTS_PER_CLUSTER == 32, "staging map");
            // A thread owns FOUR consecutive entries of cluster (tid >> 3) + 32 k: one 16-byte load of indices per thread and round,
            // n_cl / 32 rounds.  The prologue is instruction issue, not latency: a new block's waves share their SIMDs with four blocks in
            // the middle of their pixel work, and ~700 prologue instructions per thread were 6 % of a 256-light block's work, 15 % of a
            // single-light one's (block timelines, profiles/r06_i_timeline_*: "staging" 5 - 12 us whether or not the loads are batched).
            // Entries from the list's padded length (a multiple of four: one thread's share) on are never read by the walk: their threads skip the conversion.
            struct __attribute__((packed, aligned(4))) Idx4 { int32_t x, y, z, w; };
            const int part = threadIdx.x & 7;
            const float inv_tiles_x = rcp((float)tiles_x);
            for (int c = threadIdx.x >> 3; c < n_cl; c += SHADE_BLOCK / 8) {
                const int z = c & 7, t = c >> 3;
                // t / tiles_x, both <= MAX_STAGED_TILES: (t + 1/2) / tiles_x is never within 0.04 of an integer, the approximate reciprocal is exact enough
                const int ty_ = (int)(((float)t + 0.5f) * inv_tiles_x), cx = tile_x0 + (t - ty_ * tiles_x), cy = tile_y0 + ty_;
                const pbr_cluster* cl = p.clusters + (z + cx * PBR_CLUSTER_Z + cy * PBR_CLUSTER_X * PBR_CLUSTER_Z);
                const int cnt = n_lights > 0 ? min(max(cl->NumLights, 0), PBR_MAX_LIGHTS_PER_CLUSTER) : 0;
                const Idx4 v = *reinterpret_cast<const Idx4*>(cl->LightIndex + 4 * part);
                uint32_t* l = lists + c * LIST_STRIDE;
                const int padded = max((cnt + 2 * WALK_TRIPS - 1) & ~(2 * WALK_TRIPS - 1), 2 * WALK_TRIPS);
                if (4 * part < padded) {   // the thread's four entries lie below the padded count
                    auto entry = [&](int k, int raw) { return lds_base + 4u * (uint32_t)(4 * part + k < cnt ? min(max(raw, 0), n_lights - 1) : n_lights); };   // never index past the staged table
                    uint2* e = reinterpret_cast<uint2*>(l + 2 + 4 * part);   // 136 c + 8 + 16 part bytes: 8-byte aligned
                    e[0] = make_uint2(entry(0, v.x), entry(1, v.y));
                    e[1] = make_uint2(entry(2, v.z), entry(3, v.w));
                }
                if (part == 0) *reinterpret_cast<uint2*>(l) = make_uint2((uint32_t)padded, 0u);
            }
        }
    }
    __shared__ float4 s_row[SHADE_ROWS];   // the block's <= SHADE_ROWS rows
    if (threadIdx.x < (uint32_t)SHADE_ROWS)
        s_row[threadIdx.x] = shade_row_entry<STAGED_LISTS>(p, shade_row_term(p.y0 + y_begin + threadIdx.x, p.full_h), tile_y0, tiles_x);
    // bit 0: the attenuation floor cannot bind; bit 1: every staged light has the SAME attenuation polynomial (one radius for the
    // whole scene is common), so its three coefficients are per-kernel constants and a trip reads 13 LDS dwords instead of 19
    const int q_safe = (__syncthreads_and(my_safe) != 0 ? 1 : 0) | (__syncthreads_and(my_same) != 0 ? 2 : 0);
    const uint32_t px = bx0 + threadIdx.x;
    const AxisTerm col = shade_column_term(p.x0 + px, p.full_w);
    const float cvv_x = col.half_ndc * p.near_width;
    const uint32_t col_list = shade_col_list<STAGED_LISTS>(col.cluster, tile_x0);
    SHADE_ROW_LOOP(STAGED_LISTS, LSTRIDE, F32OUT, LUTFOLD);
}

// ---- shade tables (pbr_hip.h: PBR_TABLES_*) ---------------------------------------------------------------------------------------
// pbr_shade_geometry_tables: per column of the tile its shade_column_term, per row its shade_row_term, {half ndc, cluster}.  One thread per entry.
__global__ __launch_bounds__(256) void k_shade_geometry_tables(uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t full_w, uint32_t full_h, float2* __restrict__ geom) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    AxisTerm* entry = reinterpret_cast<AxisTerm*>(geom);
    if (t < w) entry[t] = shade_column_term(x0 + t, full_w);
    else if (t < w + h) entry[t] = shade_row_term(y0 + (t - w), full_h);
}

// k_deferred_shade<true, LSTRIDE, false, NoViews, true> with the prologue read from the shade tables: the light planes are a flat copy of the
// frame half's image, a tile row of the block's cluster lists is one contiguous run of it (the LDS address of the planes is added to the
// entries on the way), q_safe is the header's, the row and column terms and the block's tile bounds are look-ups in the geometry half.  One
// barrier.  LDS layout, dynamic LDS size and the row loop are k_deferred_shade's; shade_pixel is called as it is.
template <int LSTRIDE>
__global__ __launch_bounds__(SHADE_BLOCK, SHADE_MIN_WAVES) void k_deferred_shade_tabled(ShadeParams p, int n_lights, int max_clusters, ShadeRects rc, const uint32_t* __restrict__ tab) {
    __shared__ uint32_t s_mip_off[16];
    __shared__ float4 s_row[SHADE_ROWS];
    const unsigned long long t_start = SHADE_NOW();
    if (threadIdx.x < 16) s_mip_off[threadIdx.x] = p.env_mip_off[threadIdx.x];
    SHADE_LDS_CARVE(LSTRIDE);
    {   // the planes: 16 bytes per thread and round, the odd dwords behind the last whole 16 by one thread each
        constexpr int N4 = (LIGHT_PLANES * LSTRIDE) / 4, TAIL = (LIGHT_PLANES * LSTRIDE) & 3;
        const uint4* src = reinterpret_cast<const uint4*>(tab + PBR_TABLES_PLANES);
#pragma unroll 1
        for (int i = threadIdx.x; i < N4; i += SHADE_BLOCK) reinterpret_cast<uint4*>(llds)[i] = src[i];
        if (threadIdx.x < (uint32_t)TAIL) llds[4 * N4 + threadIdx.x] = __uint_as_float(tab[PBR_TABLES_PLANES + 4 * N4 + threadIdx.x]);
    }
    SHADE_BLOCK_SPAN(rc);
    // the cluster tiles of the block's rectangle: the cluster column / row of its corners (monotone in the pixel coordinate); uniform addresses
    const AxisTerm* cols = reinterpret_cast<const AxisTerm*>(tab + PBR_TABLES_GEOM);
    const AxisTerm* rows = cols + p.w;
    const uint32_t bx1 = min(bx0 + SHADE_BLOCK, x_end) - 1;
    const int tile_x0 = cols[bx0].cluster, tile_x1 = cols[bx1].cluster;
    const int ty_a = rows[y_begin].cluster, ty_b = rows[y_end - 1].cluster;
    const int tile_y0 = min(ty_a, ty_b), tile_y1 = max(ty_a, ty_b);
    const int tiles_x = tile_x1 - tile_x0 + 1;
    {
        // Tile row j of the block = clusters (tile_y0 + j, tile_x0 .. tile_x1, 0 .. 7): tiles_x * 8 lists that follow one another in the image
        // and in LDS.  16 bytes of a run per thread and round (a run starts 16-byte aligned in the image, 8-byte aligned in LDS); the four
        // dwords begin at dword 2 * (2 q mod 17) of a list, and its dwords 0 and 1 (count, pad) are not addresses.
        static_assert(LIST_STRIDE == STAGED_LIST_DWORDS && PBR_CLUSTER_Z * LIST_STRIDE % 4 == 0, "staged run");
        const int run4 = tiles_x * (PBR_CLUSTER_Z * LIST_STRIDE / 4);
        const int cap4 = max_clusters * LIST_STRIDE / 4;   // the host sized the LDS for the worst case: never past it
#pragma unroll 1   // (unrolled and vectorised the two loops were 200 static v_* for a copy that runs one or two rounds)
        for (int j = 0; j <= tile_y1 - tile_y0; j++) {
            const uint4* src = reinterpret_cast<const uint4*>(tab + PBR_TABLES_LISTS + ((tile_y0 + j) * PBR_CLUSTER_X + tile_x0) * (PBR_CLUSTER_Z * LIST_STRIDE));
            uint2* dst = reinterpret_cast<uint2*>(lists) + 2 * (j * run4);
            const int n4 = min(run4, cap4 - j * run4);
#pragma unroll 1
            for (int q = threadIdx.x; q < n4; q += SHADE_BLOCK) {
                const uint32_t m = (2u * (uint32_t)q) % 17u;
                const uint32_t lo = m == 0u ? 0u : lds_base, hi = m == 16u ? 0u : lds_base;
                const uint4 v = src[q];
                dst[2 * q] = make_uint2(v.x + lo, v.y + lo);
                dst[2 * q + 1] = make_uint2(v.z + hi, v.w + hi);
            }
        }
    }
    if (threadIdx.x < (uint32_t)SHADE_ROWS) s_row[threadIdx.x] = shade_row_entry<true>(p, rows[min(y_begin + threadIdx.x, p.h - 1u)], tile_y0, tiles_x);
    const int q_safe = (int)tab[PBR_TABLES_HEADER];
    const uint32_t px = bx0 + threadIdx.x;
    const AxisTerm col = cols[min(px, p.w - 1u)];
    const float cvv_x = col.half_ndc * p.near_width;
    const uint32_t col_list = shade_col_list<true>(col.cluster, tile_x0);
    __syncthreads();
    SHADE_ROW_LOOP(true, LSTRIDE, false, true);
}

extern "C" {

pbr_status pbr_env_pad(pbr_ctx* ctx, const pbr_half* env, uint32_t size, uint32_t mips, pbr_half* out_padded) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, env && out_padded, "pbr_env_pad: null pointer");
    PBR_REQUIRE(ctx, size >= 1 && size <= 8192 && mips >= 1 && mips <= 16 && (size >> (mips - 1)) >= 1, "pbr_env_pad: bad size/mips");
    for (uint32_t m = 0; m < mips; m++) {
        const int s = (int)(size >> m);
        const size_t n = (size_t)6 * (s + 1) * (s + 1) * 4;
        hipLaunchKernelGGL(k_env_pad, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                           env + 4 * cube_mip_offset(size, m), out_padded + 4 * env_padded_mip_offset(size, m), s);
        pbr_status r = launched(ctx, "k_env_pad");
        if (r) return r;
    }
    return PBR_OK;
}

}  // extern "C"

// The camera fields and the target fields, which ShadeParams and ShadeView name alike, are each filled by one text (the kernel's arguments
// keep the two layouts: as shared sub-structs they moved the staged kernels' scalar loads, one s_waitcnt more).  Host libm, once per call.
template <class P>
static void camera_params(const pbr_global* g, P& p) {
    camera_near_plane(g, p.InvView, p.near_width, p.near_height);
    for (int i = 0; i < 3; i++) p.CameraPos[i] = g->CameraPos[i];
    p.Near = g->Near; p.Far = g->Far;
    p.log_far_near = logf(g->Far / g->Near);
    p.inv_near = (float)(1.0 / (double)g->Near);
    p.slice_k = (float)((double)PBR_CLUSTER_Z / log2((double)g->Far / (double)g->Near));
}
template <class P>
static void target_params(P& p, const pbr_gbuffer& gb, const pbr_cluster* clusters, const pbr_light* lights, pbr_half* hdr, uint32_t hdr_pitch) {
    p.A = gb.A; p.B = gb.B; p.C = gb.C; p.depth = gb.depth; p.stencil = gb.stencil; p.pitch = gb.pitch;
    p.clusters = clusters; p.lights = lights; p.hdr = hdr; p.hdr_pitch = hdr_pitch;
}

// what every target of a launch shares: the camera of g (a view table replaces it per view), LUT and padded env chain; the rest is zero
static ShadeParams shade_params(const pbr_global* g, const pbr_half* lut, uint32_t lut_res, const pbr_half* env, uint32_t env_size, uint32_t env_mips) {
    ShadeParams p{};
    camera_params(g, p);
    p.sh = g->SkyBoxSH;
    p.lut = lut; p.lut_res = lut_res; p.env = env; p.env_size = env_size; p.env_mips = env_mips;
    for (uint32_t m = 0; m < 16; m++) p.env_mip_off[m] = (uint32_t)env_padded_mip_offset(env_size, m < env_mips ? m : env_mips - 1);
    return p;
}

// The checks of a shade launch return what is wrong (nullptr: nothing).  The tile:
static const char* shade_tile_bad(const pbr_tile* tile) {
    if (!(tile->w >= 1 && tile->h >= 1 && tile->w <= 65535 && tile->h <= 65535)) return "bad tile size";
    if (!(tile->x0 + tile->w <= tile->full_w && tile->y0 + tile->h <= tile->full_h)) return "tile outside frame";
    return nullptr;
}
// The LUT and padded env chain every target reads:
// (lut: the half2 LUT, or — lut_align 8 — its x-folded table)
static const char* shade_tables_bad(const void* lut, uint32_t lut_res, const pbr_half* env, uint32_t env_size, uint32_t env_mips, uint32_t lut_align = 4) {
    if (!lut || !env) return "null pointer";
    if (!(lut_res >= 1 && env_size >= 1 && env_mips >= 1 && env_mips <= 16 && (env_size >> (env_mips - 1)) >= 1)) return "bad LUT/env size";
    if (!(lut_res <= 16384 && (uint64_t)pbr_env_padded_texels(env_size, env_mips) * 8u < (1ull << 32)))
        return "LUT larger than 16384^2 or padded env chain of 4 GiB or more (32-bit texture offsets)";
    if (((uintptr_t)env & 7u) != 0 || ((uintptr_t)lut & (lut_align - 1u)) != 0) return lut_align == 4 ? "env must be 8-byte and lut 4-byte aligned" : "env and the folded LUT must be 8-byte aligned";
    return nullptr;
}

// one target of w x h pixels: its G-buffer, clusters, output, camera range and lights
static const char* shade_target_bad(const pbr_global* g, const pbr_gbuffer& gb, const pbr_cluster* clusters, const void* out, uint32_t out_pitch,
                                    uint32_t w, uint32_t h, const pbr_light* lights, int num_lights) {
    if (!clusters || !out) return "null pointer";
    if (!(gb.A && gb.B && gb.C && gb.depth && gb.stencil)) return "null G-buffer plane";
    if (!(gb.pitch >= w && out_pitch >= w)) return "pitch < width";
    // the kernel addresses every plane with 32-bit byte offsets (16 B per pixel for the fp32 probe's output)
    if (!((uint64_t)gb.pitch * h * 4u < (1ull << 32) && (uint64_t)out_pitch * h * 16u < (1ull << 32)))
        return "target too large for 32-bit plane offsets (pitch x rows x 16 bytes must stay below 4 GiB)";
    if (!(g->Near > 0.0f && g->Far > g->Near)) return "need 0 < Near < Far";
    if (!(num_lights >= 0 && num_lights <= PBR_MAX_SCENE_LIGHTS)) return "light count out of [0, 1024]";
    if (!(num_lights == 0 || lights != nullptr)) return "null lights";
    return nullptr;
}

// The schedule (see the kernel) of `rects` (tile-local {x, y, w, h}, checked): long blocks first, short ones for the tail.
// rc.first[rc.n] is the block count of one view; the long blocks' row count is sized for the row pieces of all n_views views.
static ShadeRects shade_schedule(const pbr_ctx* ctx, const uint32_t (*rects)[4], uint32_t n_rects, uint32_t n_views) {
    static const float big_frac = pbr::knob_float("PBR_SHADE_BIGFRAC", 0.92f);   // re-swept after the per-pixel trims (the knobs build): 0.9-0.95 with 1-row tail blocks beats 0.85 / 2 by ~0.4 %
    static const uint32_t rows_small_cfg = (uint32_t)pbr::knob_int("PBR_SHADE_ROWS_SMALL", 1);
    static const uint32_t rows_big_cfg = (uint32_t)pbr::knob_int("PBR_SHADE_ROWS_BIG", 0);   // 0: by target size (below)
    const uint32_t rows_small = rows_small_cfg >= 1 && rows_small_cfg <= (uint32_t)SHADE_ROWS ? rows_small_cfg : 1u;
    // Rows of a long block.  SHADE_ROWS (8) wherever that gives at least ~1.3 generations of the blocks the device holds at once
    // (compute units x 5): the tables a block stages are amortised best, and 4K (3.2 generations), a cfg5 rank's tile (1.7) and 8K
    // measure best there.  Smaller targets get the row count that makes ~1.6 generations — one generation and a bit (1.1) is the worst
    // place to be: the launch then lasts two block lifetimes for one block's worth of work per slot.  Measured (profiles/r06_j_rows_*,
    // r06_g_*): 1440x960 (the reference's own target, 0.56 generations at 8 rows) 3 rows -10 %; 1920x1080 (0.84) 4 rows -0.5 ... -2.4 %.
    uint64_t row_segments = 0;   // 256-pixel row pieces of the launch
    for (uint32_t r = 0; r < n_rects; r++) row_segments += (uint64_t)((rects[r][2] + SHADE_BLOCK - 1) / SHADE_BLOCK) * rects[r][3];
    row_segments *= n_views;
    uint32_t rows_big = (uint32_t)SHADE_ROWS;
    const uint64_t slots = (uint64_t)ctx->cu_count * SHADE_MIN_WAVES;
    if (row_segments * 10 < slots * 13 * SHADE_ROWS) {
        const uint32_t rws = (uint32_t)((row_segments * 10 + slots * 8) / (slots * 16));   // round(row_segments / (1.6 slots))
        rows_big = rws < 2 ? 2u : (rws > (uint32_t)SHADE_ROWS ? (uint32_t)SHADE_ROWS : rws);
    }
    if (rows_big_cfg >= 1 && rows_big_cfg <= (uint32_t)SHADE_ROWS) rows_big = rows_big_cfg;
    ShadeRects rc{};
    rc.n = n_rects; rc.rows_big = rows_big; rc.rows_small = rows_small < rows_big ? rows_small : rows_big;
    uint32_t blocks = 0;
    for (uint32_t r = 0; r < n_rects; r++) {
        const uint32_t* q = rects[r];
        rc.x0[r] = q[0]; rc.y0[r] = q[1]; rc.w[r] = q[2]; rc.h[r] = q[3];
        rc.cols[r] = (q[2] + SHADE_BLOCK - 1) / SHADE_BLOCK;
        rc.nb_big[r] = (uint32_t)((float)(q[3] / rows_big) * fminf(fmaxf(big_frac, 0.0f), 1.0f));
        const uint32_t rest = q[3] - rc.nb_big[r] * rows_big;
        rc.first[r] = blocks;
        blocks += rc.cols[r] * (rc.nb_big[r] + (rest + rc.rows_small - 1) / rc.rows_small);
    }
    rc.first[n_rects] = blocks;
    return rc;
}

// One launch of the schedule rc over n_views views (grid: rc's blocks x n_views) of a p.full_w x p.full_h frame whose views hold at most
// max_lights lights.  VS = NoViews: p is the one view's, num_lights its light count; VS = ShadeViews: every view's own fields come from vs.
template <bool F32OUT, bool LUTFOLD, class VS>
static pbr_status shade_dispatch(pbr_ctx* ctx, const ShadeParams& p, int num_lights, int max_lights, const ShadeRects& rc, uint32_t n_views, const VS& vs,
                                 const uint32_t* tables = nullptr) {
    // A block covers 256 x 8 pixels.  It can stage its cluster lists when that rectangle spans at most
    // MAX_STAGED_TILES cluster tiles: a tile is full_w/24 x full_h/16 pixels, +1 per axis for straddling.
    // The staged-list decision depends on the frame size alone; the light stride of a batch is its largest view's (a layout, not a result).
    const uint32_t span_x = (uint32_t)((uint64_t)(SHADE_BLOCK - 1) * PBR_CLUSTER_X / p.full_w) + 2;
    const uint32_t span_y = (uint32_t)((uint64_t)(SHADE_ROWS - 1) * PBR_CLUSTER_Y / p.full_h) + 2;
    const int lstride = shade_light_stride(max_lights);   // odd strides: no ds_read2 merging of two planes of one light, conflict-free planes
    const size_t plane_bytes = (size_t)((LIGHT_PLANES * lstride + 1) & ~1) * sizeof(float);
    // staged lists must also fit the 64 KiB a block may ask for (1 024 lights: 36 KiB of planes leave room for 8 tiles)
    const bool staged = span_x * span_y <= (uint32_t)MAX_STAGED_TILES &&   // (no lights at all: every list is one null pair)
                        plane_bytes + (size_t)span_x * span_y * PBR_CLUSTER_Z * LIST_STRIDE * sizeof(uint32_t) <= 65536;
    const int max_clusters = staged ? (int)(span_x * span_y) * PBR_CLUSTER_Z : 0;
    const size_t lds = plane_bytes + (size_t)max_clusters * LIST_STRIDE * sizeof(uint32_t);
    const dim3 grid(rc.first[rc.n], n_views), blk(SHADE_BLOCK);
    // one choice by (staged, stride) for both kernels; launch(staged, stride) gets them as integral constants
    auto pick = [&](auto launch) {
        auto by_stride = [&](auto st) { if (lstride == 257) launch(st, std::integral_constant<int, 257>{}); else launch(st, std::integral_constant<int, PBR_MAX_SCENE_LIGHTS + 1>{}); };
        if (staged) by_stride(std::true_type{}); else by_stride(std::false_type{});
    };
    if constexpr (std::is_same_v<VS, NoViews> && LUTFOLD && !F32OUT) {
        if (tables && staged) {   // the prologue from the shade tables (not staged: the kernel below reads lights and clusters itself)
            pick([&](auto, auto stride) { hipLaunchKernelGGL((k_deferred_shade_tabled<stride.value>), grid, blk, lds, ctx->stream, p, num_lights, max_clusters, rc, tables); });
            return launched(ctx, "k_deferred_shade_tabled");
        }
    }
    pick([&](auto st, auto stride) { hipLaunchKernelGGL((k_deferred_shade<st.value, stride.value, F32OUT, VS, LUTFOLD>), grid, blk, lds, ctx->stream, p, num_lights, max_clusters, rc, vs); });
    return launched(ctx, std::is_same_v<VS, NoViews> ? "k_deferred_shade" : "k_deferred_shade<views>");
}

// The shade tables of a launch: stale or half-built tables are refused here, on the host (the descriptor names what each half was built for)
static const char* shade_prologue_bad(const pbr_shade_tables* t, const pbr_tile* tile, int num_lights) {
    if (!t->dev) return "null tables";
    if (!((t->built & PBR_TABLES_BUILT_FRAME) && (t->built & PBR_TABLES_BUILT_GEOMETRY))) return "only one half of the tables is built";
    if (t->num_lights != num_lights) return "the tables were built for another light count";
    if (memcmp(&t->tile, tile, sizeof(pbr_tile)) != 0) return "the tables were built for another tile";
    if (t->list_pad != 2u * WALK_TRIPS) return "the cull padded the lists for another walk (SHADE_WALK_TRIPS differs between cluster.hip and shade.hip)";
    if (((uintptr_t)t->dev & 15u) != 0 || t->bytes < pbr_shade_tables_bytes(tile->w, tile->h)) return "tables buffer misaligned or too small";
    return nullptr;
}

// One single-view launch of the descriptor d (pbr_hip.h), checked; refusals go out under `who`, the entry point that was called.
// LUTFOLD: d.lut_fold is read, else d.lut.  F32OUT: the probe, which writes hdr_f32 (pitch d.hdr_pitch) and leaves d.hdr alone.
template <bool F32OUT, bool LUTFOLD>
static pbr_status shade_launch(pbr_ctx* ctx, const char* who, const pbr_shade_desc& d, float* hdr_f32 = nullptr) {
    const pbr_tile* tile = d.tile;
    PBR_CHECK(ctx, who, d.g && tile && d.gb ? nullptr : "null pointer");
    PBR_CHECK(ctx, who, d.rects || d.n_rects == 0 ? nullptr : "null rectangle list");
    PBR_CHECK(ctx, who, shade_tile_bad(tile));
    PBR_CHECK(ctx, who, shade_target_bad(d.g, *d.gb, d.clusters, F32OUT ? (const void*)hdr_f32 : (const void*)d.hdr, d.hdr_pitch, tile->w, tile->h, d.lights, d.num_lights));
    PBR_CHECK(ctx, who, shade_tables_bad(LUTFOLD ? (const void*)d.lut_fold : (const void*)d.lut, d.lut_res, d.env_padded, d.env_size, d.env_mips, LUTFOLD ? 8 : 4));
    const uint32_t whole[1][4] = {{0, 0, tile->w, tile->h}};
    const uint32_t (*rects)[4] = d.rects ? d.rects : whole;
    const uint32_t n_rects = d.rects ? d.n_rects : 1;
    PBR_CHECK(ctx, who, n_rects >= 1 && n_rects <= (uint32_t)SHADE_MAX_RECTS ? nullptr : "1 .. 5 rectangles");
    for (uint32_t r = 0; r < n_rects; r++) {
        const uint32_t* q = rects[r];
        PBR_CHECK(ctx, who, q[2] >= 1 && q[3] >= 1 && q[0] + q[2] <= tile->w && q[1] + q[3] <= tile->h ? nullptr : "rectangle outside the tile");
    }
    if (d.tables) PBR_CHECK(ctx, who, shade_prologue_bad(d.tables, tile, d.num_lights));
    ShadeParams p = shade_params(d.g, LUTFOLD ? nullptr : d.lut, d.lut_res, d.env_padded, d.env_size, d.env_mips);
    if (LUTFOLD) p.lut_fold = d.lut_fold;
    p.x0 = tile->x0; p.y0 = tile->y0; p.w = tile->w; p.h = tile->h; p.full_w = tile->full_w; p.full_h = tile->full_h;
    target_params(p, *d.gb, d.clusters, d.lights, d.hdr, d.hdr_pitch);
    p.hdr_f32 = hdr_f32;
    return shade_dispatch<F32OUT, LUTFOLD>(ctx, p, d.num_lights, d.num_lights, shade_schedule(ctx, rects, n_rects, 1), 1, NoViews{},
                                           d.tables ? (const uint32_t*)d.tables->dev : nullptr);
}

extern "C" {

pbr_status pbr_deferred_shade(pbr_ctx* ctx, const pbr_shade_desc* d) {
    if (!ctx) return PBR_ERR_INVALID;
    const char* who = "pbr_deferred_shade";
    PBR_CHECK(ctx, who, d ? nullptr : "null descriptor");
    PBR_CHECK(ctx, who, !d->lut != !d->lut_fold ? nullptr : "exactly one of lut and lut_fold");
    PBR_CHECK(ctx, who, !d->tables || d->lut_fold ? nullptr : "tables need lut_fold");
    // (the sampled form is named first: the kernels stand in the code object in the order their launches are instantiated)
    return d->lut ? shade_launch<false, false>(ctx, who, *d) : shade_launch<false, true>(ctx, who, *d);
}

// The x-folded LUT: out_fold[y][rb] (lut_res x 256 entries of two floats) = the x-lerps of LUT row y's two channels at roughness
// byte rb, exactly the fp32 values the shade's sampled form computes per pixel.  Once per LUT.
pbr_status pbr_lut_fold_x(pbr_ctx* ctx, const pbr_half* lut, uint32_t lut_res, float* out_fold) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, lut && out_fold, "pbr_lut_fold_x: null pointer");
    PBR_REQUIRE(ctx, lut_res >= 1 && lut_res <= 16384, "pbr_lut_fold_x: lut_res out of [1, 16384]");
    PBR_REQUIRE(ctx, ((uintptr_t)lut & 3u) == 0 && ((uintptr_t)out_fold & 7u) == 0, "pbr_lut_fold_x: lut must be 4-byte and the table 8-byte aligned");
    hipLaunchKernelGGL(k_lut_fold_x, dim3(lut_res), dim3(256), 0, ctx->stream, lut, (int)lut_res, out_fold);
    return launched(ctx, "k_lut_fold_x");
}

// The geometry half of the shade tables (pbr_hip.h), once per target
pbr_status pbr_shade_geometry_tables(pbr_ctx* ctx, const pbr_tile* tile, pbr_shade_tables* tables) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, tile && tables, "pbr_shade_geometry_tables: null pointer");
    PBR_CHECK(ctx, "pbr_shade_geometry_tables", shade_tile_bad(tile));
    PBR_REQUIRE(ctx, tables->dev && ((uintptr_t)tables->dev & 15u) == 0 && tables->bytes >= pbr_shade_tables_bytes(tile->w, tile->h),
                "pbr_shade_geometry_tables: the tables buffer must be 16-byte aligned and hold pbr_shade_tables_bytes(w, h)");
    tables->built &= ~PBR_TABLES_BUILT_GEOMETRY;
    hipLaunchKernelGGL(k_shade_geometry_tables, dim3((tile->w + tile->h + 255) / 256), dim3(256), 0, ctx->stream, tile->x0, tile->y0, tile->w, tile->h,
                       tile->full_w, tile->full_h, reinterpret_cast<float2*>((uint32_t*)tables->dev + PBR_TABLES_GEOM));
    const pbr_status r = launched(ctx, "k_shade_geometry_tables");
    if (r == PBR_OK) { tables->built |= PBR_TABLES_BUILT_GEOMETRY; tables->tile = *tile; }
    return r;
}

// Parity probe: the same kernel body, storing float4 instead of rounding to the R16G16B16A16_FLOAT target — what the
// <= 1e-4 relative L-inf bound of the shaded buffer is stated on.  Not a product path: the sampled whole-tile shade alone.
pbr_status pbr_deferred_shade_f32(pbr_ctx* ctx, const pbr_shade_desc* d, float* hdr_f32) {
    if (!ctx) return PBR_ERR_INVALID;
    const char* who = "pbr_deferred_shade_f32";
    PBR_CHECK(ctx, who, d ? nullptr : "null descriptor");
    PBR_CHECK(ctx, who, !d->lut_fold && !d->tables && !d->rects && d->n_rects == 0 && !d->hdr ? nullptr : "the probe takes lut alone: no lut_fold, tables, rects or hdr");
    PBR_CHECK(ctx, who, ((uintptr_t)hdr_f32 & 15u) == 0 ? nullptr : "output must be 16-byte aligned");
    return shade_launch<true, false>(ctx, who, *d, hdr_f32);
}

// DeferredShadingPass::Execute for up to PBR_MAX_VIEWS whole frames in ONE launch.  Per view exactly pbr_deferred_shade's pixels: the
// block shape does not enter a pixel's result, and the staged-list decision depends on the frame size alone.  What the batch changes:
// the long blocks' row count is sized for the whole launch (row pieces of every view), and the LDS light stride is the batch's
// largest (a layout, not a result).
pbr_status pbr_deferred_shade_views(pbr_ctx* ctx, const pbr_view* views, uint32_t n, uint32_t w, uint32_t h,
                                    const pbr_half* lut, uint32_t lut_res,
                                    const pbr_half* env, uint32_t env_size, uint32_t env_mips) {
    if (!ctx) return PBR_ERR_INVALID;
    const char* who = "pbr_deferred_shade_views";
    PBR_REQUIRE(ctx, views_count_ok(views, n), "pbr_deferred_shade_views: need 1 .. PBR_MAX_VIEWS views");
    PBR_REQUIRE(ctx, w >= 1 && h >= 1 && w <= 65535 && h <= 65535, "pbr_deferred_shade_views: bad frame size");
    PBR_CHECK(ctx, who, shade_tables_bad(lut, lut_res, env, env_size, env_mips));
    ShadeViews vs{};
    int max_lights = 0;
    for (uint32_t i = 0; i < n; i++) {
        const pbr_view& v = views[i];
        PBR_CHECK(ctx, who, shade_target_bad(&v.g, v.gb, v.clusters, v.hdr, v.hdr_pitch, w, h, v.lights, v.num_lights));
        PBR_REQUIRE(ctx, memcmp(&v.g.SkyBoxSH, &views[0].g.SkyBoxSH, sizeof(pbr_sh_pack)) == 0, "pbr_deferred_shade_views: SkyBoxSH differs between views");
        camera_params(&v.g, vs.v[i]);
        target_params(vs.v[i], v.gb, v.clusters, v.lights, v.hdr, v.hdr_pitch);
        vs.v[i].n_lights = v.num_lights;
        max_lights = v.num_lights > max_lights ? v.num_lights : max_lights;
    }
    PBR_REQUIRE(ctx, views_disjoint(views, n, 1, [&](const pbr_view& v, int, uintptr_t& lo, uintptr_t& hi) {
                    lo = addr(v.hdr); hi = lo + ((size_t)v.hdr_pitch * (h - 1) + w) * 8u; }),
                "pbr_deferred_shade_views: two views share an HDR target");
    ShadeParams p = shade_params(&views[0].g, lut, lut_res, env, env_size, env_mips);
    p.w = p.full_w = w; p.h = p.full_h = h;
    const uint32_t whole[1][4] = {{0, 0, w, h}};
    return shade_dispatch<false, false>(ctx, p, 0, max_lights, shade_schedule(ctx, whole, 1, n), n, vs);
}

}  // extern "C"
