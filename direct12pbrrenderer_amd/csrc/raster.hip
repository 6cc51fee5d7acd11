// raster.hip — the passes and data formats either side of the shade, minus the rasterizer:
//   k_skybox          skybox.hlsl:12-28         (SkyboxPass::Execute, DeferredPipeline.cpp:59-75)
//   k_skybox_bc6h     the same pass on a sky resident as the cube-map file's BC6H_UF16 blocks, sampled in place (pbr_skybox_bc6h)
//   k_gbuffer_encode  gbuffer.hlsl::ps_main :88-149  (GBufferPass::Execute, DeferredPipeline.cpp:138-185)
//   k_rgbe_decode     Radiance .hdr texels -> fp32 (ResourceLoader::LoadHDRImageFile, ResourceLoader.cpp:381-406)
// Both are streaming, HBM-bound kernels: one lane per pixel, rows contiguous across the wave.
// Built with -ffp-contract=off: same operation order as the oracle (the ray feeds floor() in the
// cube addressing, the gamma/octahedral results feed UNORM8 rounding).
#include "pbr_internal.hpp"
#include "pbr_device.hpp"
#include "tex_chain.hpp"
#include "bc6h_decode_block.hpp"
#include <type_traits>

using namespace pbr;

namespace {

struct SkyParams {
    float InvView[9];
    float near_width, near_height, Near;
    float full_w_f, full_h_f;
    uint32_t x0, y0, w, h;
    uint32_t sky_size, sky_mips;
    uint32_t pitch, hdr_pitch;
};

__device__ __forceinline__ V3 sky_ray(const SkyParams& p, float gx, float gy) {
    const float u = (gx + 0.5f) / p.full_w_f, v = (gy + 0.5f) / p.full_h_f;
    const float ndc_x = 2.0f * u - 1.0f, ndc_y = 1.0f - 2.0f * v;
    const V3 c = v3(ndc_x * 0.5f * p.near_width, ndc_y * 0.5f * p.near_height, p.Near);
    return v3(p.InvView[0] * c.x + p.InvView[1] * c.y + p.InvView[2] * c.z,
              p.InvView[3] * c.x + p.InvView[4] * c.y + p.InvView[5] * c.z,
              p.InvView[6] * c.x + p.InvView[7] * c.y + p.InvView[8] * c.z);
}

// sc/ma, tc/ma of `d` on a given face (no major-axis test): the footprint of the neighbouring
// rays is measured on the centre pixel's face
__device__ __forceinline__ void project_on_face(V3 d, uint32_t face, float& u, float& v) {
    float sc, tc, ma;
    switch (face) {
        case 0: ma = d.x;  sc = -d.z; tc = -d.y; break;
        case 1: ma = -d.x; sc = d.z;  tc = -d.y; break;
        case 2: ma = d.y;  sc = d.x;  tc = d.z;  break;
        case 3: ma = -d.y; sc = d.x;  tc = -d.z; break;
        case 4: ma = d.z;  sc = d.x;  tc = -d.y; break;
        default: ma = -d.z; sc = -d.x; tc = -d.y; break;
    }
    u = sc / ma;
    v = tc / ma;
}

// One sky pixel, whatever form the cube is resident in: SAMPLE(d, lod) is TextureCube.SampleLevel(LinearClamp, d, lod).  A macro so
// that both kernels hold this text once and k_skybox compiles to what it always did (as a function template it did not: its
// argument loads were regrouped).
#define PBR_SKYBOX_PIXEL(p, stencil, hdr, SAMPLE)                                                                   \
    const uint32_t px = blockIdx.x * 64u + (threadIdx.x & 63u);                                                     \
    const uint32_t py = blockIdx.y * 4u + (threadIdx.x >> 6);                                                       \
    if (px >= p.w || py >= p.h) return;                                                                             \
    if (stencil[(size_t)py * p.pitch + px] != 0) return;   /* geometry: the shade owns this pixel */                \
    const float gx = (float)(p.x0 + px), gy = (float)(p.y0 + py);                                                   \
    const V3 d = sky_ray(p, gx, gy);                                                                                \
    uint32_t face; float fu, fv;                                                                                    \
    cube_face_uv<true>(d, face, fu, fv);                                                                            \
    float u0, v0, ux, vx, uy, vy;                                                                                   \
    project_on_face(d, face, u0, v0);                                                                               \
    project_on_face(sky_ray(p, gx + 1.0f, gy), face, ux, vx);                                                       \
    project_on_face(sky_ray(p, gx, gy + 1.0f), face, uy, vy);                                                       \
    const float half_size = 0.5f * (float)p.sky_size;                                                               \
    const float rx = half_size * sqrtf((ux - u0) * (ux - u0) + (vx - v0) * (vx - v0));                              \
    const float ry = half_size * sqrtf((uy - u0) * (uy - u0) + (vy - v0) * (vy - v0));                              \
    const float lod = log2f(fmaxf(rx, ry));                                                                         \
    const F4 c = SAMPLE(d, lod);                                                                                    \
    store_h4(hdr + 4 * ((size_t)py * p.hdr_pitch + px), f4(c.x, c.y, c.z, 1.0f));

// pbr_skybox_views / pbr_skybox_bc6h_views: grid (.., .., views); view blockIdx.z's camera terms, stencil plane and HDR target from
// the view table, in place of p's and the arguments'.  NoViews (empty, last in the argument block: it moves no argument): the
// single-view kernel.
struct SkyView {
    float InvView[9];
    float near_width, near_height, Near;
    const uint8_t* stencil;
    pbr_half* hdr;
    uint32_t pitch, hdr_pitch;
};
struct SkyViews { SkyView v[PBR_MAX_VIEWS]; };
#define PBR_SKY_TAKE_VIEW(VS, vs, p, stencil, hdr)                                                                  \
    if constexpr (!std::is_same_v<VS, NoViews>) {                                                                   \
        const SkyView& view = vs.v[blockIdx.z];                                                                     \
        for (int i = 0; i < 9; i++) p.InvView[i] = view.InvView[i];                                                 \
        p.near_width = view.near_width; p.near_height = view.near_height; p.Near = view.Near;                       \
        p.pitch = view.pitch; p.hdr_pitch = view.hdr_pitch;                                                         \
        stencil = view.stencil; hdr = view.hdr;                                                                     \
    }

template <class VS>
__global__ __launch_bounds__(256) void k_skybox(SkyParams p, const float* __restrict__ sky,
                                                const uint8_t* __restrict__ stencil, pbr_half* __restrict__ hdr, VS vs) {
    PBR_SKY_TAKE_VIEW(VS, vs, p, stencil, hdr)
#define PBR_SKY_F32(d, lod) cube_trilinear<CubeTexelF32, true>(sky, p.sky_size, p.sky_mips, d, lod)   // the oracle's divides (pbr_device.hpp)
    PBR_SKYBOX_PIXEL(p, stencil, hdr, PBR_SKY_F32)
#undef PBR_SKY_F32
}

// unorm8, decode_gamma, pack_normal: shared with the rasterizer's resolve (gbuffer_raster.hip)
#include "gbuffer_encode.hpp"

__global__ __launch_bounds__(256) void k_gbuffer_encode(const float4* __restrict__ m0, const float4* __restrict__ m1,
                                                        const float4* __restrict__ m2, uint32_t w, uint32_t h,
                                                        uint32_t pitch, uint32_t* __restrict__ A,
                                                        uint32_t* __restrict__ B, uint32_t* __restrict__ C) {
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u);
    const uint32_t y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * pitch + x;
    const float4 a = m0[i], b = m1[i], c = m2[i];
    PBR_GBUFFER_ENCODE(a, b, c, pa, pb, pc)
    A[i] = pa; B[i] = pb; C[i] = pc;
}

// Radiance RGBE -> fp32 RGBA (4 B in, 16 B out per texel; one texel per lane, grid-stride)
__global__ __launch_bounds__(256) void k_rgbe_decode(const uint32_t* __restrict__ rgbe, size_t texels, float4* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < texels; i += (size_t)gridDim.x * 256u) {
        const uint32_t v = rgbe[i];
        const int e = (int)(v >> 24);
        // 2^(e-136) built in the exponent field (e-136+127 in [-8, 246]: subnormal scale below e = 10)
        const float scale = e ? ldexpf(1.0f, e - 136) : 0.0f;
        out[i] = make_float4((float)(v & 255u) * scale, (float)((v >> 8) & 255u) * scale, (float)((v >> 16) & 255u) * scale, 1.0f);
    }
}

// ---- the sky resident as the file's BC6H_UF16 blocks (pbr_skybox_bc6h) ----
// Everything around the texel fetch is k_skybox's: the ray, the face, the LOD, cube_lod_levels, cube_face_uv<true>, bilinear_coord,
// cube_fetch_seamless, bilerp and the level lerp of cube_trilinear.  A level's four taps lie in 1, 2 or 4 blocks of the centre face or,
// at a seam, on another face: cube_fetch_seamless runs with a policy that hands back each tap's address (face, x, y) in place of its
// colour, then every DISTINCT block among the four is read (one 16-byte load) and header-decoded once (bc6h_dec::header: the mode
// switch, the delta transform, the unquantize) and serves all the taps that lie in it (bc6h_dec::texel: one index, one weight,
// three interpolations).  The block loop and the level loop are not unrolled, so the kernel holds the fourteen mode headers once;
// a wave runs every mode its lanes hold.  The block in flight is nine words, the taps' half codes twelve: static indices and
// selects only, no private array, no LDS.
struct SkyBc6h {
    const uint4* face[6];
    uint32_t face_first[bc6h_chain::MAX_LEVELS];   // blocks of one face in front of the level: the head of bc6h_chain::Cube's table
};

struct CubeTapAddress {     // the texel policy that returns where a tap landed: the bit patterns of face, x, y (moved, never computed with)
    __device__ __forceinline__ F4 operator()(uint32_t f, int x, int y) const {
        return f4(__uint_as_float(f), __int_as_float(x), __int_as_float(y), 0.0f);
    }
};

__device__ __forceinline__ F4 bc6h_bilinear(const SkyBc6h& L, uint32_t ff, int s, V3 dir) {
    uint32_t face; float u, v;
    cube_face_uv<true>(dir, face, u, v);
    const BilinearCoord cx = bilinear_coord(u, s), cy = bilinear_coord(v, s);
    const CubeTapAddress where;
    const F4 a00 = cube_fetch_seamless(s, face, cx.i0, cy.i0, where), a10 = cube_fetch_seamless(s, face, cx.i1, cy.i0, where);
    const F4 a01 = cube_fetch_seamless(s, face, cx.i0, cy.i1, where), a11 = cube_fetch_seamless(s, face, cx.i1, cy.i1, where);
    const uint32_t bw = max(1u, ((uint32_t)s + 3u) >> 2);
    // a tap's block: face << 28 | its number in the level of that face (below 2048^2 = 2^22); its texel in the block
    uint32_t key[4], tx[4], half[4][3];
    const F4 addr[4] = {a00, a10, a01, a11};
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {
        const uint32_t f = __float_as_uint(addr[j].x), x = __float_as_uint(addr[j].y), y = __float_as_uint(addr[j].z);   // 0 <= x, y < s
        key[j] = (f << 28) | ((y >> 2) * bw + (x >> 2));
        tx[j] = 4u * (y & 3u) + (x & 3u);
        half[j][0] = half[j][1] = half[j][2] = 0u;
    }
    uint32_t todo = 15u;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; k++) {
        if (!((todo >> k) & 1u)) continue;                     // tap k lay in a block an earlier tap read
        const uint32_t kk = k == 0u ? key[0] : k == 1u ? key[1] : k == 2u ? key[2] : key[3];
        const uint32_t f = kk >> 28;
        const uint4* src = f == 0 ? L.face[0] : f == 1 ? L.face[1] : f == 2 ? L.face[2] : f == 3 ? L.face[3] : f == 4 ? L.face[4] : L.face[5];
        const uint4 q = src[ff + (kk & 0x0fffffffu)];
        const bc6h_dec::Block B = bc6h_dec::header(q.x, q.y, q.z, q.w);
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) {
            if (((todo >> j) & 1u) && key[j] == kk) {
                bc6h_dec::texel(B, tx[j], half[j]);
                todo &= ~(1u << j);
            }
        }
    }
    F4 c[4];
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++)
        c[j] = f4(bc6h_dec::half_to_f32(half[j][0]), bc6h_dec::half_to_f32(half[j][1]), bc6h_dec::half_to_f32(half[j][2]), 1.0f);
    return bilerp(c[0], c[1], c[2], c[3], cx.f, cy.f);
}

__device__ __forceinline__ F4 bc6h_trilinear(const SkyBc6h& L, uint32_t size, uint32_t mips, V3 d, float lod) {
    uint32_t l0, l1; float f;
    cube_lod_levels(mips, lod, l0, l1, f);
    const bool one = f == 0.0f || l1 == l0;
    F4 a = f4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
#pragma unroll 1
    for (uint32_t i = 0; i < 2u; i++) {
        const uint32_t l = i == 0u ? l0 : l1;
        uint32_t ff = 0;
#pragma unroll
        for (uint32_t k = 1; k < bc6h_chain::MAX_LEVELS; k++) ff = l >= k ? L.face_first[k] : ff;   // (static indices: the table stays in scalar registers)
        const F4 c = bc6h_bilinear(L, ff, (int)(size >> l), d);
        if (i == 0u) a = c; else b = c;
        if (one) break;
    }
    return one ? a : fma4(b, f, a * (1.0f - f));
}

static_assert(sizeof(SkyParams) + sizeof(SkyBc6h) + 2 * 8 + sizeof(SkyViews) <= 4096 - 256, "k_skybox<SkyViews>, k_skybox_bc6h<SkyViews>: kernel arguments over 4 KiB");

template <class VS>
__global__ __launch_bounds__(256) void k_skybox_bc6h(SkyParams p, SkyBc6h sky, const uint8_t* __restrict__ stencil, pbr_half* __restrict__ hdr,
                                                     VS vs) {
    PBR_SKY_TAKE_VIEW(VS, vs, p, stencil, hdr)
#define PBR_SKY_BC6H(d, lod) bc6h_trilinear(sky, p.sky_size, p.sky_mips, d, lod)
    PBR_SKYBOX_PIXEL(p, stencil, hdr, PBR_SKY_BC6H)
#undef PBR_SKY_BC6H
}

void fill_sky_params(SkyParams& p, const pbr_global* g, const pbr_tile* tile, uint32_t size, uint32_t mips, uint32_t pitch, uint32_t hdr_pitch) {
    camera_near_plane(g, p.InvView, p.near_width, p.near_height);
    p.Near = g->Near;
    p.full_w_f = (float)tile->full_w; p.full_h_f = (float)tile->full_h;
    p.x0 = tile->x0; p.y0 = tile->y0; p.w = tile->w; p.h = tile->h;
    p.sky_size = size; p.sky_mips = mips;
    p.pitch = pitch; p.hdr_pitch = hdr_pitch;
}

// the views of a sky resolve, checked (nullptr: usable; the caller refuses under its own name), as the kernels' table; p: what the
// views share (whole w x h frames, the cube's size)
const char* fill_sky_views(SkyParams& p, SkyViews& vs, const pbr_view* views, uint32_t n, uint32_t w, uint32_t h, uint32_t size, uint32_t mips) {
    if (!views_count_ok(views, n)) return "need 1 .. PBR_MAX_VIEWS views";
    if (!(w && h)) return "bad size";
    const pbr_tile tile{0, 0, w, h, w, h};
    for (uint32_t i = 0; i < n; i++) {
        const pbr_view& v = views[i];
        if (!(v.gb.stencil && v.hdr)) return "null pointer in a view";
        if (!(v.gb.pitch >= w && v.hdr_pitch >= w)) return "a view's pitch < width";
        fill_sky_params(p, &v.g, &tile, size, mips, v.gb.pitch, v.hdr_pitch);
        SkyView& s = vs.v[i];
        for (int k = 0; k < 9; k++) s.InvView[k] = p.InvView[k];
        s.near_width = p.near_width; s.near_height = p.near_height; s.Near = p.Near;
        s.stencil = v.gb.stencil; s.hdr = v.hdr;
        s.pitch = v.gb.pitch; s.hdr_pitch = v.hdr_pitch;
    }
    if (!views_disjoint(views, n, 1, [&](const pbr_view& v, int, uintptr_t& lo, uintptr_t& hi) {
            lo = addr(v.hdr); hi = lo + ((size_t)(h - 1) * v.hdr_pitch + w) * 8; }))
        return "two views' HDR targets overlap";
    return nullptr;
}

// the resident cube, checked (nullptr: usable), as k_skybox_bc6h takes it
const char* fill_sky_bc6h(SkyBc6h& L, const pbr_cube_bc6h* sky) {
    if (const char* why = bc6h_chain::refusal(sky->size, sky->mips)) return why;
    if (const char* why = bc6h_chain::faces_refusal(sky->face_blocks)) return why;
    bc6h_chain::Cube<const uint4*> T;             // (a face's blocks in front of a level are below 2^28: bc6h_bilinear's key)
    bc6h_chain::fill(T, sky->size, sky->mips);
    for (int f = 0; f < 6; f++) L.face[f] = static_cast<const uint4*>(sky->face_blocks[f]);
    for (uint32_t l = 0; l < bc6h_chain::MAX_LEVELS; l++) L.face_first[l] = T.face_first[l];
    return nullptr;
}

}  // namespace

extern "C" {

pbr_status pbr_rgbe_decode(pbr_ctx* ctx, const uint8_t* rgbe, size_t texels, float* out_rgba) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, rgbe && out_rgba && texels, "pbr_rgbe_decode: null pointer / empty image");
    PBR_REQUIRE(ctx, (((uintptr_t)rgbe & 3u) | ((uintptr_t)out_rgba & 15u)) == 0u, "pbr_rgbe_decode: unaligned buffer");
    size_t blocks = (texels + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_rgbe_decode, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, reinterpret_cast<const uint32_t*>(rgbe), texels,
                       reinterpret_cast<float4*>(out_rgba));
    return pbr::launched(ctx, "k_rgbe_decode");
}

pbr_status pbr_skybox(pbr_ctx* ctx, const pbr_global* g, const pbr_tile* tile, const pbr_cube_f32* sky,
                      const uint8_t* stencil, uint32_t pitch, pbr_half* hdr, uint32_t hdr_pitch) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, g && tile && sky && sky->data && stencil && hdr, "pbr_skybox: null pointer");
    PBR_REQUIRE(ctx, tile->w && tile->h && tile->full_w && tile->full_h && pitch >= tile->w && hdr_pitch >= tile->w,
                "pbr_skybox: bad tile / pitch");
    PBR_REQUIRE(ctx, sky->size && sky->mips && (sky->size >> (sky->mips - 1)) >= 1, "pbr_skybox: bad cube");
    SkyParams p;
    fill_sky_params(p, g, tile, sky->size, sky->mips, pitch, hdr_pitch);
    dim3 grid((tile->w + 63) / 64, (tile->h + 3) / 4);
    hipLaunchKernelGGL(k_skybox<NoViews>, grid, dim3(256), 0, ctx->stream, p, sky->data, stencil, hdr, NoViews{});
    return pbr::launched(ctx, "k_skybox");
}

pbr_status pbr_skybox_views(pbr_ctx* ctx, const pbr_view* views, uint32_t n, uint32_t w, uint32_t h, const pbr_cube_f32* sky) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, sky && sky->data, "pbr_skybox_views: null pointer");
    PBR_REQUIRE(ctx, sky->size && sky->mips && (sky->size >> (sky->mips - 1)) >= 1, "pbr_skybox_views: bad cube");
    SkyParams p;
    SkyViews vs{};
    PBR_CHECK(ctx, "pbr_skybox_views", fill_sky_views(p, vs, views, n, w, h, sky->size, sky->mips));
    dim3 grid((w + 63) / 64, (h + 3) / 4, n);
    hipLaunchKernelGGL(k_skybox<SkyViews>, grid, dim3(256), 0, ctx->stream, p, sky->data, (const uint8_t*)nullptr, (pbr_half*)nullptr, vs);
    return pbr::launched(ctx, "k_skybox<views>");
}

pbr_status pbr_skybox_bc6h(pbr_ctx* ctx, const pbr_global* g, const pbr_tile* tile, const pbr_cube_bc6h* sky,
                           const uint8_t* stencil, uint32_t pitch, pbr_half* hdr, uint32_t hdr_pitch) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, g && tile && sky && stencil && hdr, "pbr_skybox_bc6h: null pointer");
    PBR_REQUIRE(ctx, tile->w && tile->h && tile->full_w && tile->full_h && pitch >= tile->w && hdr_pitch >= tile->w,
                "pbr_skybox_bc6h: bad tile / pitch");
    SkyBc6h L;
    PBR_CHECK(ctx, "pbr_skybox_bc6h", fill_sky_bc6h(L, sky));
    SkyParams p;
    fill_sky_params(p, g, tile, sky->size, sky->mips, pitch, hdr_pitch);
    dim3 grid((tile->w + 63) / 64, (tile->h + 3) / 4);
    hipLaunchKernelGGL(k_skybox_bc6h<NoViews>, grid, dim3(256), 0, ctx->stream, p, L, stencil, hdr, NoViews{});
    return pbr::launched(ctx, "k_skybox_bc6h");
}

pbr_status pbr_skybox_bc6h_views(pbr_ctx* ctx, const pbr_view* views, uint32_t n, uint32_t w, uint32_t h, const pbr_cube_bc6h* sky) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, sky, "pbr_skybox_bc6h_views: null pointer");
    SkyBc6h L;
    PBR_CHECK(ctx, "pbr_skybox_bc6h_views", fill_sky_bc6h(L, sky));
    SkyParams p;
    SkyViews vs{};
    PBR_CHECK(ctx, "pbr_skybox_bc6h_views", fill_sky_views(p, vs, views, n, w, h, sky->size, sky->mips));
    dim3 grid((w + 63) / 64, (h + 3) / 4, n);
    hipLaunchKernelGGL(k_skybox_bc6h<SkyViews>, grid, dim3(256), 0, ctx->stream, p, L, (const uint8_t*)nullptr, (pbr_half*)nullptr, vs);
    return pbr::launched(ctx, "k_skybox_bc6h<views>");
}

pbr_status pbr_gbuffer_encode(pbr_ctx* ctx, const float* m0, const float* m1, const float* m2,
                              uint32_t w, uint32_t h, uint32_t pitch, uint32_t* A, uint32_t* B, uint32_t* C) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, m0 && m1 && m2 && A && B && C, "pbr_gbuffer_encode: null pointer");
    PBR_REQUIRE(ctx, w && h && pitch >= w, "pbr_gbuffer_encode: bad size");
    PBR_REQUIRE(ctx, ((((uintptr_t)m0) | ((uintptr_t)m1) | ((uintptr_t)m2)) & 15u) == 0u,
                "pbr_gbuffer_encode: material planes must be 16-byte aligned");
    dim3 grid((w + 63) / 64, (h + 3) / 4);
    hipLaunchKernelGGL(k_gbuffer_encode, grid, dim3(256), 0, ctx->stream, reinterpret_cast<const float4*>(m0),
                       reinterpret_cast<const float4*>(m1), reinterpret_cast<const float4*>(m2), w, h, pitch, A, B, C);
    return pbr::launched(ctx, "k_gbuffer_encode");
}

}  // extern "C"
