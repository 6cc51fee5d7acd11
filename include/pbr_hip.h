/*
 * pbr_hip.h — C ABI of the MI355X-native deferred-PBR shading path.
 *
 * This is the drop-in boundary for the DeferredRendering HLSL compute / full-screen
 * passes of zrlhahaha/Direct12PBRRenderer.  The reference has no FFI: its seam is
 * D3D12CommandList::Dispatch(ShadingState*, gx, gy, gz) / DrawScreen(ShadingState*)
 * (Engine/Include/Renderer/Device/Direct12/D3D12CommandList.h:83,103).  Every entry
 * point below replaces ONE reference dispatch (cited per function); the C++ pass
 * classes under direct12pbrrenderer_amd/host/ call them from their Execute() bodies.
 *
 * Conventions
 *  - all image/buffer pointers are DEVICE pointers to linear, row-major planes;
 *  - every call enqueues on the context's stream and returns immediately
 *    (pbr_sync() blocks); a context is NOT thread-safe (one recording thread, as the
 *    reference: Engine/Source/App.cpp:370-377);
 *  - return value: 0 = ok, <0 = error (text via pbr_last_error);
 *  - "half" storage is IEEE binary16 in a uint16_t (R16G16_FLOAT / R16G16B16A16_FLOAT
 *    targets of the reference), RGBA8 planes are one uint32_t per pixel, R in the low
 *    byte (DXGI_FORMAT_R8G8B8A8_UNORM memory order).
 */
#ifndef PBR_HIP_H
#define PBR_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int pbr_status;
enum {
    PBR_OK              =  0,
    PBR_ERR_INVALID     = -1,  /* bad argument (null pointer, zero size, limits exceeded) */
    PBR_ERR_HIP         = -2,  /* HIP runtime error, see pbr_last_error                    */
    PBR_ERR_NOMEM       = -3,
    PBR_ERR_UNSUPPORTED = -4,
    PBR_ERR_COMM        = -5   /* RCCL error                                               */
};

typedef struct pbr_ctx pbr_ctx;
typedef uint16_t pbr_half;

/* ---- constants the reference hard-codes (kept in sync by hand there) ------------------ */
#define PBR_CLUSTER_X              24   /* DeferredRendering/Shader/clustered.hlsli:10-12   */
#define PBR_CLUSTER_Y              16
#define PBR_CLUSTER_Z              8
#define PBR_MAX_LIGHTS_PER_CLUSTER 32   /* clustered.hlsli:9                                */
#define PBR_MAX_SCENE_LIGHTS       1024 /* Engine/Include/Renderer/Pipeline/DeferredPipeline.h:329 */
#define PBR_NUM_CLUSTERS           (PBR_CLUSTER_X * PBR_CLUSTER_Y * PBR_CLUSTER_Z)
#define PBR_HISTOGRAM_BINS         256  /* DeferredPipeline.h:409                           */
#define PBR_SAMPLE_COUNT           1024 /* precompute_brdf.hlsl:3, env_map_gen.hlsl:3       */
#define PBR_ENV_MIPS               5    /* global.hlsli:9 PREFILTER_ENVMAP_MIPMAP_SIZE      */
#define PBR_BLOOM_STEP             3    /* DeferredPipeline.h:211                           */
#define PBR_BLOOM_MIPS             5    /* DeferredPipeline.h:212                           */

/* ---- POD mirrors of reference structs -------------------------------------------------- */

/* SH2CoefficientsPack, Engine/Include/Utils/SH.h:20-29 (7 x float4 = 112 B). */
typedef struct pbr_sh_pack {
    float sha_r[4], shb_r[4], sha_g[4], shb_g[4], sha_b[4], shb_b[4], shc[4];
} pbr_sh_pack;

/* ConstantBufferGlobal, Engine/Include/Renderer/Pipeline/IPipeline.h:38-62 == HLSL cbuffer
 * GlobalConstant, global.hlsli:38-57.  Matrices row-major, mul(M, v) = M*v (column vector). */
typedef struct pbr_global {
    pbr_sh_pack SkyBoxSH;
    float InvView[16];
    float View[16];
    float Projection[16];
    float InvProjection[16];
    float CameraPos[3];
    float Ratio;
    float Resolution[2];
    float Near;
    float Far;
    float Fov;
    float DeltaTime;
    float Time;
} pbr_global;                       /* 412 bytes */

/* PointLight, DeferredPipeline.h:341-347 / clustered.hlsli:31-37 (44 B). */
typedef struct pbr_light {
    float Position[3];
    float Color[3];
    float Intensity;
    float Radius, C0, C1, C2;       /* PointLightAttenuation, Scene.h:115-124 */
} pbr_light;

/* Cluster, DeferredPipeline.h:333-339 / clustered.hlsli:15-21 (156 B). */
typedef struct pbr_cluster {
    float MinBound[3];
    float MaxBound[3];
    int32_t NumLights;
    int32_t LightIndex[PBR_MAX_LIGHTS_PER_CLUSTER];
} pbr_cluster;

/* A tile of a larger frame (new: multi-GPU split).  Planes passed with a tile
 * cover w x h pixels (tile-local addressing); uv, the camera ray and ClusterIndex use the
 * GLOBAL pixel (x0 + x, y0 + y) of a full_w x full_h frame.  Single GPU: {0,0,W,H,W,H}. */
typedef struct pbr_tile {
    uint32_t x0, y0, w, h, full_w, full_h;
} pbr_tile;

/* G-buffer as written by gbuffer.hlsl::ps_main (gbuffer.hlsl:10-26,144-146); formats
 * DeferredPipeline.h:107-110.  A: rgb albedo (linear), a emission.  B: rg octahedral normal.
 * C: r roughness, g metallic, b AO.  depth: D32 in [0,1].  stencil > 0 <=> geometry.
 * pitch = row pitch in pixels of every plane. */
typedef struct pbr_gbuffer {
    const uint32_t* A;
    const uint32_t* B;
    const uint32_t* C;
    const float*    depth;
    const uint8_t*  stencil;
    uint32_t        pitch;
} pbr_gbuffer;

/* fp32 RGBA cube with a mip chain: mips concatenated (mip 0 first); inside a mip the six
 * faces +X,-X,+Y,-Y,+Z,-Z; each face row-major [y][x][4].  size = mip-0 edge. */
typedef struct pbr_cube_f32 {
    const float* data;
    uint32_t size;
    uint32_t mips;
} pbr_cube_f32;

/* ---- layout helpers (pure host functions) ----------------------------------------------- */
/* texels (not bytes) in a cube with `mips` levels */
size_t pbr_cube_texels(uint32_t size, uint32_t mips);
/* texel offset of (mip, face 0) */
size_t pbr_cube_mip_offset(uint32_t size, uint32_t mip);
/* texels of the "padded" prefiltered-env layout pbr_deferred_shade samples — a FOOTPRINT layout: for every bilinear
 * footprint origin (x, y) in [-1, s-1]^2 of every face of every mip, the four texels (x,y), (x+1,y), (x,y+1), (x+1,y+1),
 * each already resolved by the seamless-cube rule, stored together (32 contiguous bytes): the per-pixel trilinear fetch
 * is branch-free and touches ONE cache line per level.  4 x the plain chain (67 MB at 512^2 x 5).  Entry (face, y+1, x+1)
 * of mip m starts at texel pbr_env_padded_mip_offset(size, m) + ((face * (s+1) + y+1) * (s+1) + x+1) * 4. */
size_t pbr_env_padded_texels(uint32_t size, uint32_t mips);
size_t pbr_env_padded_mip_offset(uint32_t size, uint32_t mip);
/* texels of a PBR_BLOOM_MIPS-level 2D chain of a w x h image (level l is (w>>l) x (h>>l)) */
size_t pbr_bloom_chain_texels(uint32_t w, uint32_t h);
size_t pbr_bloom_level_offset(uint32_t w, uint32_t h, uint32_t level);

/* ---- context ------------------------------------------------------------------------------ */
pbr_status  pbr_ctx_create(int hip_device, pbr_ctx** out);
void        pbr_ctx_destroy(pbr_ctx* ctx);
/* enqueue on an existing hipStream_t (e.g. torch's current stream).  NULL selects HIP's default
 * (null) stream.  A new context starts on a private non-blocking stream. */
pbr_status  pbr_ctx_set_stream(pbr_ctx* ctx, void* hip_stream);
/* go back to the context's private stream */
pbr_status  pbr_ctx_use_own_stream(pbr_ctx* ctx);
/* the hipStream_t the next call will enqueue on (for a host that orders its own events / copies with the context's
 * work: the C++ pass graph records its per-frame fence there); NULL = HIP's default stream */
void*       pbr_ctx_get_stream(const pbr_ctx* ctx);
/* A second, high-priority stream of the context.  _begin: it waits for everything enqueued so far, and the calls made
 * until _end enqueue on it; _end: back to the context's stream — what follows runs concurrently with the side stream's
 * work; _join: the context's stream waits for the side stream.  (Multi-GPU: the tile's border ring and its halo exchange
 * on the side stream, the tile's core on the main one.) */
pbr_status  pbr_ctx_side_begin(pbr_ctx* ctx);
pbr_status  pbr_ctx_side_end(pbr_ctx* ctx);
pbr_status  pbr_ctx_side_join(pbr_ctx* ctx);
/* Bloom, the two large 2x-up levels of frames above ~1.6 Mpixel (levels of >= 400 tiles of 128 x 32): by default they run in polyphase
 * form — not the shader's operation order: <= 1 fp16 ULP per stage, <= 2 for the chain — so a whole frame and a smaller tile of it (which
 * takes the shader-order kernels) agree to 2 fp16 ULP, not bit for bit.  on != 0: every level in the shader's operation order
 * (k_blur_hv), bit-identical to the staged dispatches at any size — for hosts that compare tiles with frames or frames across sizes;
 * costs the polyphase form's gain (~2 % of a 4K frame). */
pbr_status  pbr_ctx_set_bloom_shader_order(pbr_ctx* ctx, int on);
const char* pbr_last_error(const pbr_ctx* ctx);
/* Which kernels ran: the context keeps the labels of its last PBR_LAUNCH_LOG kernel launches (host side only: no allocation, nothing
 * on the device).  Returns the number of launches since the context was created and stores the labels of the last
 * min(cap, PBR_LAUNCH_LOG, that number) of them in out, oldest first (out may be null: the count alone).  A label is the kernel's
 * name, with the instance where an entry point chooses between several: "k_blur_hv/16" and "k_blur_hv/32" (the tile height),
 * "k_blur_up_poly", "k_blur_hv/16<views>" ...; the strings are static. */
#define PBR_LAUNCH_LOG 64
uint64_t    pbr_launch_log(const pbr_ctx* ctx, const char** out, uint32_t cap);
/* blocks until everything enqueued through the context is done: its stream AND side-stream work not joined yet */
pbr_status  pbr_sync(pbr_ctx* ctx);
const char* pbr_version(void);
/* NULL, or why this process cannot use the library: a second ROCm installation is mapped next to the HIP runtime in
 * use (PyTorch ships its own libamdhip64; it must be loaded first).  pbr_ctx_create refuses with
 * PBR_ERR_UNSUPPORTED in that case and prints this text. */
const char* pbr_runtime_error(void);
/* the rule behind pbr_runtime_error as a pure function: 1 iff the HIP runtime in use (mapped from hip_dir) is not the
 * one PyTorch (libtorch_hip.so in torch_dir) ships — i.e. torch_dir holds its own libamdhip64.so and hip_dir is another
 * directory.  A PyTorch built against the system ROCm (no bundled runtime) is NOT a mismatch. */
int pbr_runtime_mismatch_dirs(const char* hip_dir, const char* torch_dir);

/* ---- one-shot IBL precompute --------------------------------------------------------------- */
/* precompute_brdf.hlsl:20-62 dispatched by PrecomputeBRDFPass::Execute (DeferredPipeline.cpp:117-136).
 * out: res*res half2, row-major [y][x]; x -> roughness, y -> NdotV. */
pbr_status pbr_brdf_lut(pbr_ctx* ctx, uint32_t res, pbr_half* out_rg);

/* Radiance RGBE texels (R, G, B mantissas + shared exponent, 4 bytes) -> fp32 RGBA, alpha 1: the per-texel half of
 * DirectX::LoadFromHDRFile as called by ResourceLoader::LoadHDRImageFile (ResourceLoader.cpp:381-406; DirectXTex
 * is an un-vendored, unpinned vcpkg dependency).  Published rule (G. Ward, "Real Pixels", Graphics Gems II):
 * e == 0 -> 0, else channel = mantissa * 2^(e - 136).  The file-level parse (header, scanline RLE) is host work
 * (host/HdrImage.h). */
pbr_status pbr_rgbe_decode(pbr_ctx* ctx, const uint8_t* rgbe, size_t texels, float* out_rgba);

/* 2x2 box mips of an fp32 RGBA cube in place (stands in for DirectXTex GenerateMipMaps,
 * ResourceLoader.cpp:465-507).  cube->data mip 0 must be filled; mips 1.. are written. */
pbr_status pbr_cube_gen_mips(pbr_ctx* ctx, float* cube_data, uint32_t size, uint32_t mips);

/* ---- BC6H sky cubes (new): the reference's load-time decode of a CubeMapResource ---------------------------------------- */
/* The reference serializes every HDR texture as DXGI_FORMAT_BC6H_UF16 (TextureCompression.h:13-14, BasicStorage.h:10-11): a sky
 * asset is six such chains (ResourceDef.cpp:187-219, BasicStorage.cpp:161-188) that DirectX::Decompress expands at load time.
 * One face's chain, the payload of the file byte for byte: level i is max(1, ((size >> i) + 3) / 4)^2 blocks of 16 bytes,
 * row-major, levels concatenated from level 0; texel (x, y) of a level is texel (x & 3, y & 3) of block (x >> 2, y >> 2), so a
 * block that overhangs a level smaller than 4 contributes its top-left texels.  Bytes of one face's chain; 0 for what
 * pbr_bc6h_decode_cube refuses (size 0, not a multiple of 4 or above PBR_BC6H_MAX_SIZE, mip_levels 0 or above floor(log2(size)) + 1). */
#define PBR_BC6H_MAX_SIZE 8192u   /* the largest cube pbr_cube_gen_mips, pbr_prefilter_env and pbr_sh9_project take */
size_t pbr_bc6h_chain_bytes(uint32_t size, uint32_t mip_levels);
/* face_blocks: HOST array of six DEVICE pointers, 16-byte aligned, one chain each, in the reference's face order px, nx, py, ny,
 * pz, nz (= +X, -X, +Y, -Y, +Z, -Z of pbr_cube_f32) — six pointers because in the file the chains are separated by 16-byte
 * headers; every payload of a file uploaded as it is is 16-byte aligned relative to the file's start, so it decodes in place.
 * out_rgba: DEVICE, 16-byte aligned, the pbr_cube_f32 layout of `size` and `mip_levels` (pbr_cube_texels float4 texels: mips
 * concatenated, six faces per mip), alpha 1.0f.  One asynchronous launch on the context's stream for all faces and levels, no
 * allocation, no host synchronisation.  Refusals (PBR_ERR_INVALID, nothing enqueued): a null or misaligned pointer (the array,
 * any face, out_rgba), size 0, not a multiple of 4 (the reference asserts it: BasicStorage.h:252-260) or above
 * PBR_BC6H_MAX_SIZE, mip_levels 0 or above floor(log2(size)) + 1.
 * The decode rule, pinned: the D3D11 BC6H_UF16 definition with DirectXTex's rounding term (what the reference's DirectX::Decompress
 * runs); tests/bc6h_ref.py restates it in numpy, is held to a third-party decoder on the CPU, and the kernel is held to it bit for bit.
 *   A block is 128 bits, bit 0 = the LSB of byte 0.  Mode: bits 0-1 if they are 0 or 1, otherwise bits 0-4.  The header follows, its
 *   fields in this order, LSB first; x[a:b] with a > b stores bit b first, r0[10:11] and r0[10:15] store the HIGH bit first.
 *   Two regions (endpoint bits, delta bits of r.g.b); the 5-bit partition follows at bits 77-81, 46 index bits from bit 82:
 *     0x00 10.5.5.5: g2[4] b2[4] b3[4] r0[9:0] g0[9:0] b0[9:0] r1[4:0] g3[4] g2[3:0] g1[4:0] b3[0] g3[3:0] b1[4:0] b3[1] b2[3:0] r2[4:0] b3[2] r3[4:0] b3[3]
 *     0x01 7.6.6.6:  g2[5] g3[4] g3[5] r0[6:0] b3[0] b3[1] b2[4] g0[6:0] b2[5] b3[2] g2[4] b0[6:0] b3[3] b3[5] b3[4] r1[5:0] g2[3:0] g1[5:0] g3[3:0] b1[5:0] b2[3:0] r2[5:0] r3[5:0]
 *     0x02 11.5.4.4: r0[9:0] g0[9:0] b0[9:0] r1[4:0] r0[10] g2[3:0] g1[3:0] g0[10] b3[0] g3[3:0] b1[3:0] b0[10] b3[1] b2[3:0] r2[4:0] b3[2] r3[4:0] b3[3]
 *     0x06 11.4.5.4: r0[9:0] g0[9:0] b0[9:0] r1[3:0] r0[10] g3[4] g2[3:0] g1[4:0] g0[10] g3[3:0] b1[3:0] b0[10] b3[1] b2[3:0] r2[3:0] b3[0] b3[2] r3[3:0] g2[4] b3[3]
 *     0x0a 11.4.4.5: r0[9:0] g0[9:0] b0[9:0] r1[3:0] r0[10] b2[4] g2[3:0] g1[3:0] g0[10] b3[0] g3[3:0] b1[4:0] b0[10] b2[3:0] r2[3:0] b3[1] b3[2] r3[3:0] b3[4] b3[3]
 *     0x0e 9.5.5.5:  r0[8:0] b2[4] g0[8:0] g2[4] b0[8:0] b3[4] r1[4:0] g3[4] g2[3:0] g1[4:0] b3[0] g3[3:0] b1[4:0] b3[1] b2[3:0] r2[4:0] b3[2] r3[4:0] b3[3]
 *     0x12 8.6.5.5:  r0[7:0] g3[4] b2[4] g0[7:0] b3[2] g2[4] b0[7:0] b3[3] b3[4] r1[5:0] g2[3:0] g1[4:0] b3[0] g3[3:0] b1[4:0] b3[1] b2[3:0] r2[5:0] r3[5:0]
 *     0x16 8.5.6.5:  r0[7:0] b3[0] b2[4] g0[7:0] g2[5] g2[4] b0[7:0] g3[5] b3[4] r1[4:0] g3[4] g2[3:0] g1[5:0] g3[3:0] b1[4:0] b3[1] b2[3:0] r2[4:0] b3[2] r3[4:0] b3[3]
 *     0x1a 8.5.5.6:  r0[7:0] b3[1] b2[4] g0[7:0] b2[5] g2[4] b0[7:0] b3[5] b3[4] r1[4:0] g3[4] g2[3:0] g1[4:0] b3[0] g3[3:0] b1[5:0] b2[3:0] r2[4:0] b3[2] r3[4:0] b3[3]
 *     0x1e 6.6.6.6:  r0[5:0] g3[4] b3[0] b3[1] b2[4] g0[5:0] g2[5] b2[5] b3[2] g2[4] b0[5:0] g3[5] b3[3] b3[5] b3[4] r1[5:0] g2[3:0] g1[5:0] g3[3:0] b1[5:0] b2[3:0] r2[5:0] r3[5:0]   (not transformed)
 *   One region; 63 index bits from bit 65:
 *     0x03 10.10: r0[9:0] g0[9:0] b0[9:0] r1[9:0] g1[9:0] b1[9:0]   (not transformed)
 *     0x07 11.9:  r0[9:0] g0[9:0] b0[9:0] r1[8:0] r0[10] g1[8:0] g0[10] b1[8:0] b0[10]
 *     0x0b 12.8:  r0[9:0] g0[9:0] b0[9:0] r1[7:0] r0[10:11] g1[7:0] g0[10:11] b1[7:0] b0[10:11]
 *     0x0f 16.4:  r0[9:0] g0[9:0] b0[9:0] r1[3:0] r0[10:15] g1[3:0] g0[10:15] b1[3:0] b0[10:15]
 *   The 5-bit values 0x13, 0x17, 0x1b, 0x1f are reserved: rgb = 0, alpha 1.
 *   Transformed modes (all but 0x03 and 0x1e): e_i = (e_0 + signextend(e_i, delta bits)) & (2^endpoint bits - 1), i = 1 .. 3 (one region:
 *   i = 1).  Unquantize, n = endpoint bits: n >= 15 -> x; x = 0 -> 0; x = 2^n - 1 -> 0xFFFF; otherwise ((x << 15) + 0x4000) >> (n - 1).
 *   Partitions of the two-region modes, shapes 0 .. 31, texel 0 (row-major) first, '1' = the second endpoint pair e2 / e3:
 *     0011001100110011 0001000100010001 0111011101110111 0001001100110111 0000000100010011 0011011101111111 0001001101111111 0000000100110111
 *     0000000000010011 0011011111111111 0000000101111111 0000000000010111 0001011111111111 0000000011111111 0000111111111111 0000000000001111
 *     0000100011101111 0111000100000000 0000000010001110 0111001100010000 0011000100000000 0000100011001110 0000000010001100 0111001100110001
 *     0011000100010000 0000100010001100 0110011001100110 0011011001101100 0001011111101000 0000111111110000 0111000110001110 0011100110011100
 *   Anchor texel of the second region: 15 for shapes 0 .. 16, then 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2; texel 0 is always an
 *   anchor; an anchor's index has one bit fewer (its high bit is 0).  Indices, texels 0 .. 15 in order: 3 bits with the weights 0, 9, 18,
 *   27, 37, 46, 55, 64 (two regions), 4 bits with 0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64 (one region).
 *   Interpolate and finish with the region's pair (a, b) and weight w: x = (a (64 - w) + b w + 32) >> 6; half bits = (x * 31) >> 6;
 *   the fp32 value is that half, exactly (at most 0x7BFF: never inf or NaN).  The + 32 is DirectXTex's BC67_WEIGHT_ROUND.
 * Parity with a reference-held file is not pinned: the checkout holds none (Asset/SkyBox/HDRWild.json without its data file). */
pbr_status pbr_bc6h_decode_cube(pbr_ctx* ctx, const void* const face_blocks[6], uint32_t size, uint32_t mip_levels, float* out_rgba);
/* ---- BC6H sky import (new): the producing half — ResourceLoader::ImportCubeMap's TextureCompressor::Compress to BC6H_UF16 ---- */
/* The inverse of pbr_bc6h_decode_cube, same layouts on both sides (ResourceLoader.cpp:279-299: LoadCubeMap, CubeMapTextureData,
 * BinarySerialize, Compress).  cube_rgba: DEVICE, 16-byte aligned, the pbr_cube_f32 chain of `size` and `mip_levels` (mips
 * concatenated, six faces per mip, fp32 RGBA; alpha is ignored).  face_blocks_out: HOST array of six DEVICE pointers, 16-byte
 * aligned, each receiving pbr_bc6h_chain_bytes(size, mip_levels) bytes, order px, nx, py, ny, pz, nz; nothing is written outside
 * those bytes.  One asynchronous launch on the context's stream for all faces and levels, no allocation, no host synchronisation.
 * Refusals (PBR_ERR_INVALID, nothing enqueued): those of pbr_bc6h_decode_cube — a null or misaligned pointer (the array, any face,
 * cube_rgba), size 0, not a multiple of 4 or above PBR_BC6H_MAX_SIZE, mip_levels 0 or above floor(log2(size)) + 1.
 * The encoding rule, pinned, all in integers after the first step (`/` is FLOOR division; per-texel errors fit uint32, block sums
 * and the least-squares terms are 64-bit); tests/bc6h_encode_ref.py restates it in numpy and the kernel is held to it bit for bit.
 * Only one-region modes are emitted (the two-region ones: pbr_bc6h_encode_cube_ex below).
 *   Half code of a channel value v: h = the IEEE half bit pattern of clamp(v, 0, 65504) rounded to nearest even.  NaN gives 0; any
 *   v <= 0 gives 0, -0.0 included (the sign bit is cleared); +inf and anything above 65504 give 0x7BFF; subnormal halves stay
 *   subnormal codes.  Its target in 16-bit endpoint space is t = (64 h + 30) / 31, the least x whose decode finish (31 x) >> 6 is h.
 *   A block's texels are those of the level that lie inside it (n of them, 1 .. 16: levels of 2 and 1 texels, and of 6 or 3 under a
 *   size of 12, give partial blocks).  A texel outside the level takes no part in any minimum, maximum, sum or error and gets index 0.
 *   fit(a, b) of two 16-bit endpoint triples: palette entry k = 0 .. 15 of channel c is p_k,c = ((a_c (64 - w_k) + b_c w_k + 32) >> 6)
 *   * 31 >> 6 with the 4-bit weights w_k of the decode rule; each texel takes the k of least sum_c (p_k,c - h_c)^2 (distance in
 *   half-code space), the lowest k on ties; the block's error is the sum over its texels.
 *   Start: per channel lo_c and hi_c of t over the block; dom = the channel with the largest hi - lo (the first of r, g, b on ties);
 *   cov_c = n sum(t_c t_dom) - sum(t_c) sum(t_dom); A_c = hi_c and B_c = lo_c, exchanged for every channel with cov_c < 0; fit(A, B).
 *   Refine, at most twice, at 16 bits: per texel alpha = 64 - w[index], beta = w[index]; Saa = sum(alpha alpha), Sbb = sum(beta beta),
 *   Sab = sum(alpha beta), Sat_c = sum(alpha t_c), Sbt_c = sum(beta t_c), det = Saa Sbb - Sab Sab.  det == 0: stop.  A'_c =
 *   clamp((128 (Sbb Sat_c - Sab Sbt_c) + det) / (2 det), 0, 65535), B'_c = clamp((128 (Saa Sbt_c - Sab Sat_c) + det) / (2 det), 0,
 *   65535); fit(A', B'): if its error is strictly smaller it replaces A, B, the indices and the error, otherwise stop.
 *   Modes, tried in the order 0x0f (16.4), 0x0b (12.8), 0x07 (11.9), 0x03 (10.10), n = endpoint bits: qa = A >> (16 - n), qb = B >>
 *   (16 - n); fit the pair unquantized by the decode rule.  If texel 0's index is >= 8, exchange qa and qb and replace every inside
 *   texel's index by 15 - index (the weights are symmetric: the error is unchanged).  For the three transformed modes the stored
 *   delta qb - qa must fit the mode's signed delta width in every channel AFTER that exchange, otherwise the mode is no candidate;
 *   0x03 always is.  The candidate of least error is kept, the earlier one on ties.
 *   Emit in the bit layout of the decode rule, the delta in two's complement of its width.  The anchor's high bit is always 0, no
 *   reserved mode is emitted, no texel can decode above 0x7BFF, and a block of one colour is lossless through mode 0x0f.
 * BC6H_SF16 and parity with DirectXTex's encoder (what the reference's import runs) are out of scope; the two-region modes are
 * behind pbr_bc6h_encode_cube_ex's flag. */
pbr_status pbr_bc6h_encode_cube(pbr_ctx* ctx, const float* cube_rgba, uint32_t size, uint32_t mip_levels, void* const face_blocks_out[6]);
/* pbr_bc6h_encode_cube with flags.  flags == 0: the same kernel, the same bytes.  PBR_BC6H_ENCODE_TWO_REGION: a block may also take one
 * of the ten two-region modes, by the rule below (a second kernel, k_bc6h_encode_cube2; one launch as well).  Any other bit is
 * refused (PBR_ERR_INVALID, nothing enqueued), as is everything pbr_bc6h_encode_cube refuses.  What it writes is read by
 * pbr_bc6h_decode_cube and pbr_skybox_bc6h like any other chain.
 * The two-region rule, pinned; it extends the rule above and reuses its pieces unchanged (half code, t, partial blocks, the start,
 * the refinement formulas, "strictly smaller replaces, the earlier keeps a tie"); all integers, `/` is FLOOR division;
 * tests/bc6h_encode2_ref.py restates it in numpy and the kernel is held to it bit for bit.
 *   1. The one-region result: the rule above as it is.  If its error is 0 it is emitted and nothing below runs.
 *   2. fit3(a, b, mask): fit with the 3-bit weights 0, 9, 18, 27, 37, 46, 55, 64 (palette entries k = 0 .. 7) over the texels of
 *      `mask` — a region of a shape, intersected with the level —, the lowest k on ties, the same distance; its error is the sum
 *      over those texels.
 *   3. Shape search, shapes 0 .. 31 in order.  For each of the shape's two regions: over its texels inside the level, the start of
 *      the rule above (lo and hi of t, dom, the covariance signs, n = the number of those texels) gives (A, B), and the region's
 *      estimate is fit3(A, B, region)'s error.  A region with no texel inside the level has A = B = 0 and estimate 0.  The shape's
 *      estimate is the sum of the two; the shape of least estimate is chosen, the lowest number on ties.  (Region 0 is never empty:
 *      texel 0 is in it and inside every level.)
 *   4. Refinement of the chosen shape, region by region: the start's fit3, then at most two refinements at 16 bits by the formulas
 *      above with alpha = 64 - w3[index], beta = w3[index] and the sums over the region's texels; det == 0 stops that region; a
 *      refinement replaces the region's pair, indices and error only if the region's error falls strictly, otherwise that region
 *      stops.  A region 1 with no texel inside the level then takes region 0's pair (e2 = e0, e3 = e1).
 *   5. Modes, tried in the order 0x00, 0x01, 0x02, 0x06, 0x0a, 0x0e, 0x12, 0x16, 0x1a, 0x1e, n = the mode's endpoint bits: all four
 *      endpoints >> (16 - n); each region fit3 on its pair unquantized by the decode rule; the candidate's error is the sum of the
 *      two.  Region 0: if texel 0's index is >= 4, e0 and e1 are exchanged and the index of every texel of region 0 inside the level
 *      becomes 7 - index.  Region 1: the same with the shape's anchor texel and e2, e3 (an anchor outside the level has index 0 and
 *      never exchanges).  For the nine transformed modes the stored deltas e1 - e0, e2 - e0, e3 - e0, taken AFTER the exchanges,
 *      must each fit the signed width of their channel in that mode, otherwise the mode is no candidate; 0x1e always is.
 *   6. The one-region result stays unless a two-region candidate's error is strictly smaller; among those the earlier keeps a tie.
 *   7. Emit in the bit layout of the decode rule: the header, the shape at bits 77 .. 81, 46 index bits from bit 82 (both anchors
 *      store two bits, the other texels three; a texel outside the level 0), the deltas in two's complement of their width.
 *   No reserved mode is emitted, no texel decodes above 0x7BFF, both anchors' high bits are 0.  One shape is searched past the
 *   estimate; BC6H_SF16 and parity with DirectXTex's encoder stay out of scope. */
#define PBR_BC6H_ENCODE_TWO_REGION 1u
pbr_status pbr_bc6h_encode_cube_ex(pbr_ctx* ctx, const float* cube_rgba, uint32_t size, uint32_t mip_levels, void* const face_blocks_out[6],
                                   uint32_t flags);

/* ---- Equirectangular panoramas (new): one latitude-longitude HDR image -> level 0 of a sky cube ------------------------------- */
/* The reference imports a sky from six face images only (ResourceLoader.cpp:408-428); nearly every HDR sky in circulation is one
 * equirectangular .hdr.  pbr_equirect_to_cube resamples such a panorama into level 0 of a pbr_cube_f32, the step in front of
 * pbr_cube_gen_mips, pbr_sh9_project and pbr_bc6h_encode_cube_ex.
 * pano: DEVICE, ph rows of pw texels, tightly packed, row 0 the top (+Y): fp32 RGBA (16 bytes a texel, 16-byte aligned; alpha is not
 * read) or, with PBR_EQUIRECT_SRC_RGBE, Radiance RGBE texels (4 bytes, 4-byte aligned) that are decoded by pbr_rgbe_decode's rule
 * where they are fetched: that decode is exact, so the output equals bit for bit that of the fp32 image pbr_rgbe_decode makes of the
 * same bytes, and no 16-byte-per-texel copy of the panorama exists (8192 x 4096: 134 MB instead of 537 MB).
 * cube_level0: DEVICE, 16-byte aligned, six faces px, nx, py, ny, pz, nz of size^2 float4 each (level 0 of a pbr_cube_f32); alpha
 * is written as 1.0f; nothing is written outside those 6 size^2 texels.  size need not be a multiple of 4 or a power of two (those
 * are demands of the later steps).  One asynchronous launch on the context's stream for all six faces, no allocation, no host
 * synchronisation.
 * Refusals (PBR_ERR_INVALID, nothing enqueued, the reason in pbr_last_error): a null pointer; pw, ph or size zero; pw above
 * PBR_EQUIRECT_MAX_W or ph above PBR_EQUIRECT_MAX_H; size above PBR_BC6H_MAX_SIZE; samples not one of 1, 2, 4, 8; any flag bit other
 * than PBR_EQUIRECT_SRC_RGBE; cube_level0 not 16-byte aligned; pano not aligned to its texel.
 * The rule, pinned (this project's own: nothing of DirectXTex is involved); all arithmetic is fp32, every operation written below
 * rounds once and none is fused except where fmaf says so; tests/equirect_ref.py restates it in numpy in float64 and float32 and the
 * kernel is held to the float64 form within a derived bound (tests/equirect_cases.py).  n = size * samples.  For output texel
 * (face f, x, y) and sub-sample (i, j), 0 <= i, j < samples, j the outer loop:
 *   1. Face coordinates from integers, one rounding each: a = float(2 (x samples + i) + 1 - n) / float(n), b likewise from y and j.
 *      (Not 2 (...) / size - 1: its cancellation makes the longitude ill-conditioned beside the poles.)
 *   2. Direction d = the cube's own face mapping, not normalised: f = 0 .. 5: (1, -b, -a), (-1, -b, a), (a, 1, b), (a, -1, -b),
 *      (a, -b, 1), (-a, -b, -1).
 *   3. Angles: lambda = atan2f(d.x, d.z), and 0 when d.x and d.z are both zero (of either sign); theta = atan2f(sqrtf(d.x d.x +
 *      d.z d.z), d.y) (not acos, which loses half the bits at the poles).  The panorama's centre column looks along +Z, its columns
 *      advance towards +X (to the right for a camera looking down +Z with +Y up in this left-handed frame), row 0 is +Y.
 *   4. Panorama coordinates: s = (lambda * I2 + 0.5f) * float(pw) - 0.5f, t = (theta * I1) * float(ph) - 0.5f with I2 and I1 the fp32
 *      values nearest 1 / (2 pi) and 1 / pi.
 *   5. Taps: x0 = floor(s), fx = s - x0, y0 = floor(t), fy = t - y0; columns x0 mod pw and (x0 + 1) mod pw (longitude wraps), rows
 *      clamp(y0, 0, ph - 1) and clamp(y0 + 1, 0, ph - 1) (latitude clamps: no tap crosses a pole).
 *   6. Sample, per channel r, g, b: three lerps fmaf(w, q - p, p) — row y0 along x with fx, row y0 + 1 along x with fx, then those
 *      two along y with fy.  The taps are used as they are: non-finite and negative texels follow IEEE (a zero weight does not
 *      switch a tap off: 0 * inf is NaN), nothing is clamped.
 *   7. Texel: the samples^2 samples are added in the order above (starting from 0), then multiplied by 1 / samples^2, which is exact.
 * atan2f is the device library's (OpenCL allows it 6 ulp), so the kernel is held to the rule within a bound, not bit for bit. */
#define PBR_EQUIRECT_MAX_W 16384u
#define PBR_EQUIRECT_MAX_H 8192u
#define PBR_EQUIRECT_SRC_RGBE 1u   /* pano is Radiance RGBE texels (4 bytes) instead of fp32 RGBA (16 bytes) */
pbr_status pbr_equirect_to_cube(pbr_ctx* ctx, const void* pano, uint32_t pw, uint32_t ph,
                                float* cube_level0, uint32_t size, uint32_t samples, uint32_t flags);
/* What an import picks when its caller names no cube size or sub-sample count (pure host functions): the largest power of two
 * <= pw / 4 clamped to [4, PBR_BC6H_MAX_SIZE]; the smallest of 1, 2, 4, 8 with 4 size samples >= pw, and 8 if none is. */
uint32_t pbr_equirect_default_size(uint32_t pw);
uint32_t pbr_equirect_default_samples(uint32_t pw, uint32_t size);

/* env_map_gen.hlsl:50-105, all PBR_ENV_MIPS dispatches of PreFilterEnvMapPass::Execute
 * (DeferredPipeline.cpp:77-115): mip i is filtered with roughness i/(mips-1).
 * out: half4 cube chain, layout as pbr_cube_f32 with edge `size`.
 * Mips >= 1 are sampled from a half-precision copy of the source chain WHEN THAT COPY IS EXACT — every rgb texel of every
 * source mip survives fp32 -> half -> fp32 bit for bit, which is the case for everything the reference can feed this pass (its
 * sky assets are BC6H_UF16, BasicStorage.h:10-11, and pbr_bc6h_decode_cube turns every texel of such an asset into the fp32 image
 * of a half) — and from the fp32 chain otherwise (e.g. the box mips pbr_cube_gen_mips makes); decided on the device, the call stays
 * asynchronous.  Either way <= 1 fp16 ULP (or 1e-3 relative) from the shader's sequential sum.
 * The per-mip GGX sample tables depend on (size, mips, sky->mips) only: the context keeps the last set on the device, so the FIRST
 * call with a new shape builds and uploads them (a blocking copy, ~0.2 ms of host work) and later calls do not; like every entry
 * point, one call at a time per context. */
pbr_status pbr_prefilter_env(pbr_ctx* ctx, const pbr_cube_f32* sky, uint32_t size, uint32_t mips,
                             pbr_half* out_rgba);
/* ONE dispatch of env_map_gen.hlsl: cbuffer {Roughness, MipLevel, PrefilterEnvMapTextureSize}
 * (DeferredPipeline.h:46-51).  out_mip_rgba: the 6 x (size>>mip_level)^2 half4 texels of that mip. */
pbr_status pbr_prefilter_env_mip(pbr_ctx* ctx, const pbr_cube_f32* sky, uint32_t size, uint32_t mip_level,
                                 float roughness, pbr_half* out_mip_rgba);

/* Build the padded copy of a prefiltered env chain (one-shot, after pbr_prefilter_env).
 * env_rgba: plain half4 cube chain (pbr_cube_f32 layout); out_padded: pbr_env_padded_texels half4. */
pbr_status pbr_env_pad(pbr_ctx* ctx, const pbr_half* env_rgba, uint32_t size, uint32_t mips, pbr_half* out_padded);

/* SHBaker::ProjectEnvironmentMap + PackCubeMapSHCoefficient (Engine/Source/Utils/SH.cpp:87-153,
 * 201-222) as a deterministic solid-angle quadrature over every mip-0 texel.
 * out_pack: DEVICE pointer to 28 floats (pbr_sh_pack). */
pbr_status pbr_sh9_project(pbr_ctx* ctx, const pbr_cube_f32* sky, float* out_pack);

/* ---- per-frame passes ----------------------------------------------------------------------- */
/* clustered_compute.hlsl:18-42 (ClusteredPass::Execute, DeferredPipeline.cpp:253).
 * g: HOST pointer (copied into kernel arguments).  clusters: device, PBR_NUM_CLUSTERS. */
pbr_status pbr_cluster_build(pbr_ctx* ctx, const pbr_global* g, pbr_cluster* clusters);

/* clustered_culling.hlsl:18-41 (DeferredPipeline.cpp:256).  lights: device, n <= 1024. */
pbr_status pbr_cluster_cull(pbr_ctx* ctx, const pbr_global* g, const pbr_light* lights, int n,
                            pbr_cluster* clusters);
/* both dispatches of ClusteredPass::Execute (DeferredPipeline.cpp:253-256) in one launch: bounds + light lists;
 * same results as pbr_cluster_build followed by pbr_cluster_cull */
pbr_status pbr_clustered(pbr_ctx* ctx, const pbr_global* g, const pbr_light* lights, int num_lights,
                         pbr_cluster* clusters);

/* The x-folded split-sum LUT.  The x side of the shade's bilinear LUT sample (coordinate snap, clamps, the lerp of the two taps of a
 * row) depends on the pixel's roughness BYTE and on the LUT alone: out_fold[(y * 256 + rb) * 2 + {0, 1}] holds, for LUT row y and
 * roughness byte rb, the fp32 x-lerp of each of the LUT's two channels — evaluated by the very device functions the shade calls per
 * pixel, so a shade that reads them does the y-lerp alone and gets the same bits.  Once per LUT (lut_res <= 16384);
 * out_fold: device, lut_res * 256 * 2 floats (1 MiB for a 512^2 LUT, the LUT's own size), 8-byte aligned. */
pbr_status pbr_lut_fold_x(pbr_ctx* ctx, const pbr_half* lut, uint32_t lut_res, float* out_fold);

/* ---- shade tables: what every block of the shade would otherwise derive again in its prologue ------------------------------
 * One device buffer of pbr_shade_tables_bytes(w, h) bytes (16-byte aligned) in two halves, and a HOST descriptor that names what
 * the halves were built for.  Dword offsets into the buffer:
 *   PBR_TABLES_HEADER  4 dwords: {q_safe, num_lights, light stride, 0}.  q_safe bit 0: every light has C0 >= 1e-6, C1 >= 0, C2 >= 0;
 *                      bit 1: every light has light 0's attenuation polynomial.  Stride: 257 up to 256 lights, else 1025.
 *   PBR_TABLES_PLANES  9 planes of `stride` floats (position xyz, Color * Intensity rgb, C0 C1 C2); the null light
 *                      {1e15, 1e15, 1e15, 0, 0, 0, 1, 0, 0} at index num_lights, zeros behind it.
 *   PBR_TABLES_LISTS   PBR_NUM_CLUSTERS lists of 34 dwords in the pbr_cluster table's order: padded count, 0, 32 entries.  An entry is
 *                      4 * light index; entries from the cluster's count on are 4 * num_lights (the null light).  The padded count is
 *                      the count rounded up to a multiple of list_pad (four as shipped: one step of the shade's walk), at least list_pad.
 *   PBR_TABLES_GEOM    w columns {ndc_x * 0.5f, cluster column (int)} then h rows {ndc_y * 0.5f, cluster row (int)} of the tile, from
 *                      the float expressions of the shade itself (IEEE divide, floor, clamp).
 * The frame half (header, planes, lists) is written by pbr_clustered_tables, the geometry half by pbr_shade_geometry_tables. */
#define PBR_TABLES_HEADER 0u
#define PBR_TABLES_PLANES 4u
#define PBR_TABLES_LISTS  9232u     /* 4 + 9 * 1025 rounded up to four dwords */
#define PBR_TABLES_GEOM   113680u   /* + 3072 * 34 */
#define PBR_TABLES_BUILT_FRAME 1u
#define PBR_TABLES_BUILT_GEOMETRY 2u
typedef struct pbr_shade_tables {
    void* dev;           /* the device buffer */
    uint64_t bytes;      /* its size */
    uint32_t built;      /* PBR_TABLES_BUILT_* of the halves built so far (0 before the first builder ran) */
    int32_t num_lights;  /* light count of the frame half */
    uint32_t list_pad;   /* entries the frame half's list counts are padded to (the shade refuses tables padded for another walk) */
    pbr_tile tile;       /* tile of the geometry half */
} pbr_shade_tables;
size_t pbr_shade_tables_bytes(uint32_t w, uint32_t h);

/* pbr_clustered that also writes the frame half of `tables` (same launch: the wave that culls a cluster writes its staged list,
 * one more block writes the light planes and the header) and records num_lights in the descriptor.  clusters: as pbr_clustered. */
pbr_status pbr_clustered_tables(pbr_ctx* ctx, const pbr_global* g, const pbr_light* lights, int num_lights,
                                pbr_cluster* clusters, pbr_shade_tables* tables);

/* The geometry half of `tables` for `tile` (one-shot per target, like pbr_lut_fold_x per LUT); records the tile in the descriptor. */
pbr_status pbr_shade_geometry_tables(pbr_ctx* ctx, const pbr_tile* tile, pbr_shade_tables* tables);

/* deferred_shading.hlsl:91-192 full-screen pass, stencil-masked (DeferredPipeline.cpp:187-206): ONE launch described by a HOST struct
 * (pointers first, then the 32-bit fields: no padding).
 * gb: HOST struct of device planes.  env_padded: the PADDED half4 cube chain produced by pbr_env_pad (the fixed-function seamless-cube
 * addressing, done once instead of per tap).
 * lut / lut_fold: exactly one is set.  lut: the lut_res x lut_res half2 LUT, sampled per pixel.  lut_fold: pbr_lut_fold_x's table of that
 * LUT (8-byte aligned): the same HDR target bit for bit, ~33 VALU instructions less per pixel.
 * lights / num_lights: the PointLights buffer the cluster lists index (num_lights <= 1024; the kernel stages exactly num_lights records
 * into LDS, indices are clamped to that range).
 * hdr: tile-local w x h half4, pitch hdr_pitch pixels; untouched where stencil == 0.
 * rects / n_rects: NULL, 0 shades the whole tile; else 1 .. 5 rectangles of it (tile-local {x, y, w, h}), pixels outside are left
 * untouched.  The overlapped multi-GPU frame shades the tile's border ring first (<= 4 rectangles), starts the halo exchange of its
 * bloom strips, and shades the core while they travel.
 * tables: NULL, or the shade tables (needs lut_fold): the blocks copy their light planes, cluster lists, row and column terms from them
 * instead of deriving them, the same HDR target bit for bit.  PBR_ERR_INVALID unless both halves are built, for this tile and this
 * num_lights.  `lights` and `clusters` must be the ones pbr_clustered_tables was given; targets too small to stage cluster lists per
 * block run the kernel that reads them directly.
 * Limits (32-bit offsets inside the kernel, PBR_ERR_INVALID beyond them): pitch x tile rows x 16 bytes < 4 GiB per plane,
 * lut_res <= 16384, padded env chain < 4 GiB (env_size <= 4096 with a full mip chain). */
typedef struct pbr_shade_desc {
    const pbr_global* g;
    const pbr_tile* tile;
    const pbr_gbuffer* gb;
    const pbr_half* lut;
    const float* lut_fold;
    const pbr_half* env_padded;
    const pbr_cluster* clusters;
    const pbr_light* lights;
    pbr_half* hdr;
    const uint32_t (*rects)[4];
    const pbr_shade_tables* tables;
    uint32_t lut_res;
    uint32_t env_size, env_mips;
    int32_t num_lights;
    uint32_t hdr_pitch;
    uint32_t n_rects;
} pbr_shade_desc;
pbr_status pbr_deferred_shade(pbr_ctx* ctx, const pbr_shade_desc* d);

/* Parity probe (not a product path): the same shade, storing the fp32 colour (float4 per pixel, alpha 1, pitch d->hdr_pitch pixels,
 * 16-byte aligned) instead of rounding it to the half4 target — the buffer the <= 1e-4 relative L-inf parity bound is stated on.
 * d->hdr must be NULL; lut_fold, tables and rects are refused (the probe is the sampled whole-tile shade). */
pbr_status pbr_deferred_shade_f32(pbr_ctx* ctx, const pbr_shade_desc* d, float* hdr_f32);

/* ---- SURVEY 8f "next" rows: the two raster passes either side of the shade, minus rasterization ---- */
/* skybox.hlsl:12-28 (SkyboxPass::Execute, DeferredPipeline.cpp:59-75): the sky sphere is drawn at the far
 * plane with depth test and no depth write, i.e. it lands exactly on the pixels geometry did not cover
 * (stencil == 0).  hdr(px) = SkyBox.Sample(LinearWrap, camera ray through px).rgb, alpha 1; pixels with
 * stencil > 0 are left untouched (the shade overwrites them).  The sampler's implicit LOD is defined as
 * log2 of the larger forward-difference footprint (in mip-0 texels) of the ray on the centre pixel's face. */
pbr_status pbr_skybox(pbr_ctx* ctx, const pbr_global* g, const pbr_tile* tile, const pbr_cube_f32* sky,
                      const uint8_t* stencil, uint32_t pitch, pbr_half* hdr, uint32_t hdr_pitch);
/* The same pass on a sky that stays resident as the file's BC6H_UF16 blocks (1 byte per texel instead of the 16 of pbr_cube_f32): the
 * blocks are sampled in place, each texel decoded by the rule pinned at pbr_bc6h_decode_cube.  face_blocks: six DEVICE pointers,
 * 16-byte aligned, one chain of pbr_bc6h_chain_bytes(size, mips) bytes each, order px, nx, py, ny, pz, nz — the addresses
 * pbr_bc6h_decode_cube takes, e.g. the payloads of a cube-map file uploaded as it is.
 * The HDR target is bit-identical to pbr_skybox on the cube pbr_bc6h_decode_cube makes of the same chains; pixels with stencil != 0
 * are untouched.  One asynchronous launch on the context's stream, no allocation, no host synchronisation.
 * Refusals (PBR_ERR_INVALID, nothing enqueued): those of pbr_skybox (a null pointer, an empty tile, pitch or hdr_pitch below the
 * tile's width) and those of pbr_bc6h_decode_cube on the chains: a null or non-16-byte-aligned face, size 0, not a multiple of 4 or
 * above PBR_BC6H_MAX_SIZE, mips 0 or above floor(log2(size)) + 1. */
typedef struct pbr_cube_bc6h { const void* face_blocks[6]; uint32_t size, mips; } pbr_cube_bc6h;   /* DEVICE pointers, order px … nz */
pbr_status pbr_skybox_bc6h(pbr_ctx* ctx, const pbr_global* g, const pbr_tile* tile, const pbr_cube_bc6h* sky,
                           const uint8_t* stencil, uint32_t pitch, pbr_half* hdr, uint32_t hdr_pitch);

/* gbuffer.hlsl::ps_main :88-149 without the rasterizer / texture fetches: per-pixel material attributes ->
 * G-buffer planes.  m0 = (albedo.rgb as authored (gamma space), emission), m1 = (normal_ws.xyz, roughness),
 * m2 = (metallic, ambient occlusion, -, -): three float4 planes of pitch `pitch` pixels.
 * A = UNORM8(decode_gamma(albedo), emission), B = UNORM8(octahedral(normalize(n)), 1, 0),
 * C = UNORM8(roughness, metallic, ao, 0)  (global.hlsli:73-77,101-133; formats DeferredPipeline.h:107-109). */
pbr_status pbr_gbuffer_encode(pbr_ctx* ctx, const float* m0, const float* m1, const float* m2,
                              uint32_t w, uint32_t h, uint32_t pitch, uint32_t* A, uint32_t* B, uint32_t* C);

/* ---- G-buffer rasterization (new): triangle meshes with constant per-draw materials -> the five G-buffer planes ---------- */
/* VSInput_P3F_N3F_T2F_T2F (DeferredRendering/Shader/global.hlsli:59-66), 56 B: the reference's vertex buffers pass through
 * unchanged.  The raster reads position and normal only (the textured raster also tangent and uv). */
typedef struct pbr_vertex {
    float position[3];
    float normal[3];
    float tangent[3];
    float color[3];
    float uv[2];
} pbr_vertex;
/* ConstantBufferInstance (gbuffer.hlsl:33-48) without the Use*Map flags (every draw takes the constant-material branches),
 * plus the draw's index range: triangles are indices[first_index + 3 i .. + 2] + base_vertex, i < index_count / 3.
 * Model / InvModel row-major, mul(M, v) = M v (as pbr_global).  164 B. */
typedef struct pbr_draw {
    float Model[16];
    float InvModel[16];
    float Albedo[3];               /* as authored (gamma space): decode_gamma is applied */
    float Emission;
    float Roughness;
    float Metallic;
    uint32_t first_index;
    uint32_t index_count;
    int32_t  base_vertex;
} pbr_draw;
#define PBR_RASTER_MAX_DRAWS     65536u
#define PBR_RASTER_MAX_TRIANGLES (1u << 22)
#define PBR_RASTER_MAX_SIZE      8192u   /* full_w, full_h */
/* Scratch of pbr_gbuffer_raster for a w x h tile and n_triangles triangles: the recommended size (per-bin triangle lists for
 * about 8 bins per triangle), and the minimum.  Any size from the minimum up gives the same bits.  Bins take list space in raster
 * order while their list fits (and holds <= 2048 triangles); a bin without a list walks EVERY triangle record: its cost grows with
 * bins x triangles.  The minimum holds no lists at all — every bin walks every triangle — and is meant for tests and small scenes,
 * not for large ones (a 4K tile of 4 M triangles would read 32 400 x 4 M records). */
size_t pbr_gbuffer_raster_scratch_bytes(uint32_t w, uint32_t h, uint32_t n_triangles);
size_t pbr_gbuffer_raster_min_scratch_bytes(uint32_t w, uint32_t h, uint32_t n_triangles);
/* pbr_gbuffer_raster, ONE call described by a HOST struct, pbr_raster_desc; both are declared below, after the types of the optional
 * fields.  This block is the contract of every call; the two after it say what `maps` and `bounds` add.
 * GBufferPass::Execute + DrawModel (DeferredPipeline.cpp:138-185) for constant-material draws: gbuffer.hlsl's vertex shader
 * (position_ws = Model (p, 1), normal_ws = transpose(InvModel) (n, 0), clip = Projection (View position_ws); g->View and
 * g->Projection), DefaultOpaque's fixed-function state and ps_main's Use*Map == false branches (AO = 0).  Draws run in array order.
 *   Clears: A = B = C = 0, depth = 1, stencil = 0.  Viewport (0, 0, full_w, full_h), depth range [0, 1].
 *   Clipping: near plane (z >= 0) in clip space; x / y only outside a guard band of 128 w.  Vertices snap to 1/256 pixel
 *   (round to nearest even).  Coverage: exact integer edge functions at pixel centres, top-left rule; back faces (counter-
 *   clockwise in y-down screen space) and zero-area triangles are dropped.  Depth: z / w linear in screen space, clamped to [0, 1],
 *   test LESS with write; stencil counts the depth-passing fragments (INCR_SAT).  A / B / C: the first fragment in draw order
 *   that reaches the pixel's nearest depth; its normal interpolated perspective-correctly, encoded as pbr_gbuffer_encode.
 *   Accuracy of the interpolated attributes (the normal here; tangent and uv with d->maps): the barycentrics come from the
 *   triangle's 2D homogeneous edge planes, formed in fp64 about an integer pixel origin within the triangle's on-screen bounding box and
 *   rounded once to fp32, evaluated in fp32 at the pixel's exact offset from that origin.  Their error is a few 2^-24 of sum |lambda_i|
 *   (4-5 at the median, about 20 at worst for well-shaped triangles; the bound per pixel is derived in tests/raster_truth.py) and does
 *   not depend on where the tile or the triangle lies in the frame, up to PBR_RASTER_MAX_SIZE; the origin is a function of the
 *   triangle and the frame only, so tiles stay bit-identical to the frame.
 *   Accuracy of coverage and depth: against the real-number geometry of the float32 clip coordinates (homogeneous edge functions, the
 *   near-plane line, depth = sum lambda_i z_i / det) a pixel's verdict can differ only within delta of a line, delta = the line's ends'
 *   displacement along its normal at the pixel's foot point: the snap's 1/512 pixel per axis, 3 * 2^-24 (|x / w| + 1) full_w / 2 of the
 *   projection, and a float32 intersection for an end on the near plane or the guard band (2.8e-3 pixel for an unclipped triangle);
 *   depth lies within |d depth / dx| e_x + |d depth / dy| e_y + a few 2^-24 of that geometry's.  The bound is derived and evaluated
 *   per pixel in tests/raster_cover_truth.py; measured there, verdicts differ up to 0.28 delta from a line and depth uses up to 0.95 of
 *   its band (numpy restatement and MI355X alike).
 * tile: the planes hold global pixels (x0 + x, y0 + y) of the full_w x full_h frame, w x h of them at row pitch `pitch` pixels; a
 * tile is bit-identical to the same region of the whole frame, for every scratch size.
 * vertices / indices / draws: DEVICE arrays of n_vertices / n_indices / n_draws.  max_triangles: the triangles the draws hold
 * (sum of index_count / 3), which the scratch is sized for; triangles past it are not drawn.  Guard on device data: a draw
 * whose range passes n_indices, or a triangle with an index + base_vertex outside [0, n_vertices), is dropped.
 * Limits (PBR_ERR_INVALID, nothing enqueued): n_draws <= PBR_RASTER_MAX_DRAWS, max_triangles <= PBR_RASTER_MAX_TRIANGLES,
 * full_w, full_h <= PBR_RASTER_MAX_SIZE; null pointers, zero counts, a tile outside its frame, pitch < w, scratch below
 * pbr_gbuffer_raster_min_scratch_bytes(w, h, max_triangles), buffers not 4-byte (scratch: 16-byte) aligned are refused.
 * A null descriptor is refused too.  Asynchronous: six launches on the context's stream, no host synchronisation, no allocation. */

/* ---- Textured G-buffer rasterization (new): gbuffer.hlsl's Use*Map == true branches ------------------------------------- */
/* A 2D texture with its whole mip chain in device memory, as the reference creates it (ResourceDef.cpp:53-66, TextureInfo and
 * CalculateMipmapLayout, BasicStorage.h:193-233): level i is (width >> i) x (height >> i) texels, rows tightly packed, levels
 * concatenated from level 0.  format: the DXGI number, one of the four the reference's assets use. */
#define PBR_TEX_R8G8B8A8_UNORM       28u
#define PBR_TEX_B8G8R8A8_UNORM       87u
#define PBR_TEX_B8G8R8A8_UNORM_SRGB  91u
#define PBR_TEX_R8_UNORM             61u
#define PBR_TEX_MAX_SIZE             16384u
/* BC1-resident chains: PBR_TEX_BC1_BLOCKS ORed into `format` says that `texels` holds the chain as BC1 blocks, the payload of the
 * reference's *_data.bin texture files byte for byte (what TextureDecompressInternal, TextureCompression.cpp, decodes at load
 * time), and format & 0xff is the stored format the reference would decode it into.  Level i is max(1, ((width >> i) + 3) / 4) x
 * max(1, ((height >> i) + 3) / 4) blocks of 8 bytes, row-major within a level, levels concatenated from level 0; texel (x, y) of a
 * level is texel (x & 3, y & 3) of block (x >> 2, y >> 2), so a level smaller than a block uses the block's top-left texels.
 * The BC1 decode rule (the format's public definition), pinned: a block is two little-endian uint16 endpoints c0, c1 (RGB565: red
 * in bits 15-11, green 10-5, blue 4-0) and 16 2-bit indices, texel (x, y) in bits 2 (4 y + x) + 1 .. 2 (4 y + x) of the little-
 * endian uint32 that follows.  Endpoints expand to 8 bits by bit replication ((c5 << 3) | (c5 >> 2), (c6 << 2) | (c6 >> 4)).
 * c0 > c1 (as uint16): index 0 = c0, 1 = c1, 2 = (2 c0 + c1 + 1) / 3, 3 = (c0 + 2 c1 + 1) / 3 per channel (integer division), alpha
 * 255.  Otherwise: 0 = c0, 1 = c1, 2 = (c0 + c1 + 1) / 2, alpha 255, and 3 = transparent black (0, 0, 0, 0).  Stored bytes per
 * format: 28 R, G, B, A; 87 and 91 B, G, R, A; 61 R.  The decode applies or removes no sRGB curve: format 91's curve is the
 * sampler's (below), as for a decoded chain. */
#define PBR_TEX_BC1_BLOCKS           0x100u
typedef struct pbr_texture2d {
    const void* texels;            /* device; 4-byte aligned for the 4-byte formats; BC1 blocks: 8-byte aligned */
    uint32_t width, height;        /* 1 .. PBR_TEX_MAX_SIZE */
    uint32_t mip_levels;           /* 1 .. floor(log2(min(width, height))) + 1 */
    uint32_t format;               /* PBR_TEX_*, optionally | PBR_TEX_BC1_BLOCKS */
} pbr_texture2d;
/* Bytes of a whole chain of either kind (format with or without PBR_TEX_BC1_BLOCKS); 0 for a description pbr_gbuffer_raster
 * would refuse (a zero size or one above PBR_TEX_MAX_SIZE, mip_levels out of range, an unknown stored format, any other bit of format). */
size_t pbr_texture2d_bytes(uint32_t width, uint32_t height, uint32_t mip_levels, uint32_t format);
/* The reference's load-time decode (TextureDecompressInternal) of a whole chain on the GPU: blocks (device, 8-byte aligned, the
 * BC1 layout above) -> out (device, the uncompressed layout of pbr_texture2d in stored_format, pbr_texture2d_bytes(width, height,
 * mip_levels, stored_format) bytes; 4-byte aligned for the 4-byte formats), by the rule pinned above.  One asynchronous launch on
 * the context's stream for all levels, no allocation.  Refusals (PBR_ERR_INVALID, nothing enqueued): a null pointer, misaligned
 * blocks or out, a zero size or one above PBR_TEX_MAX_SIZE, mip_levels 0 or above floor(log2(min(w, h))) + 1, stored_format not
 * one of the four (PBR_TEX_BC1_BLOCKS included: the flag describes the input, not the output). */
pbr_status pbr_bc1_decode(pbr_ctx* ctx, const void* blocks, uint32_t width, uint32_t height, uint32_t mip_levels,
                          uint32_t stored_format, void* out);
/* ---- Texture import (new): the producing half — ResourceLoader::ImportTexture's GenerateImageMipmaps and TextureCompressor::Compress ---- */
/* The mip chain of a 2D texture, in place like pbr_cube_gen_mips: texels (device) is a chain in the uncompressed pbr_texture2d layout
 * of `format` (one of the four stored formats, without PBR_TEX_BC1_BLOCKS; 4-byte aligned for the 4-byte formats) with level 0
 * filled; levels 1 .. mip_levels - 1 are written.  The rule, pinned (the one of every fixture chain, scene.mip_chain): texel (x, y)
 * of level l, (width >> l) x (height >> l), is per stored byte (a + b + c + d + 2) >> 2 of the texels (2x, 2y), (2x + 1, 2y),
 * (2x, 2y + 1), (2x + 1, 2y + 1) of level l - 1 as that level was rounded; an odd last row / column of the level above is dropped;
 * no sRGB curve is applied or removed (format 91 averages its stored bytes).  Asynchronous on the context's stream, no allocation,
 * no host synchronisation, at most two launches: one block per 64 x 64 tile of level 0 takes it down levels 1 .. 6 (the 2 x 2
 * footprints are aligned at every level), a second launch of one block makes levels 7 and up from level 6.  mip_levels == 1 is
 * valid and enqueues nothing.  Refusals (PBR_ERR_INVALID, nothing enqueued): null or misaligned texels, a zero size or one above
 * PBR_TEX_MAX_SIZE, mip_levels 0 or above floor(log2(min(w, h))) + 1, format not one of the four (any other bit set included). */
pbr_status pbr_texture2d_gen_mips(pbr_ctx* ctx, void* texels, uint32_t width, uint32_t height, uint32_t mip_levels, uint32_t format);
/* The inverse of pbr_bc1_decode, same argument order, same layouts on both sides: texels (device, the uncompressed chain in
 * stored_format; 4-byte aligned for the 4-byte formats) -> blocks_out (device, 8-byte aligned, the BC1 chain exactly as
 * PBR_TEX_BC1_BLOCKS defines it: pbr_texture2d_bytes(width, height, mip_levels, stored_format | PBR_TEX_BC1_BLOCKS) bytes).  One
 * asynchronous launch on the context's stream for all levels, no allocation.  Refusals (PBR_ERR_INVALID, nothing enqueued): those
 * of pbr_bc1_decode (stored_format | PBR_TEX_BC1_BLOCKS included: the flag describes the output, not the input).
 * The encoding rule, pinned, all in integers (every intermediate fits a signed 32-bit integer; `/` on possibly negative numerators
 * is FLOOR division); tests/bc1_encode_ref.py restates it in numpy and the kernel is held to it bit for bit:
 *   Texel -> (r, g, b): format 28 the stored R, G, B; 87 and 91 the swizzle (stored B, G, R); 61 (r, r, r).  Stored alpha is
 *   ignored; every emitted texel decodes with alpha 255.  No sRGB curve.
 *   A block's texels are those of the level that lie inside it (n of them, 1 .. 16: a level smaller than a block, or one whose size
 *   is no multiple of 4, gives partial blocks, the "top-left texels" of PBR_TEX_BC1_BLOCKS).  A texel outside the level takes no
 *   part in any minimum, maximum or sum below and gets index 0.
 *   Start: per channel c, lo_c and hi_c over the block; dom = the channel with the largest hi_c - lo_c (the first of r, g, b on
 *   ties); cov_c = n sum(x_c x_dom) - sum(x_c) sum(x_dom).  Endpoint A_c = hi_c and B_c = lo_c, exchanged for every channel with
 *   cov_c < 0.  Quantise (v an 8-bit channel): 5 bits (31 v + 127) / 255 for red and blue, 6 bits (63 v + 127) / 255 for green; the
 *   RGB565 word is r5 << 11 | g6 << 5 | b5.
 *   Fit of a pair of RGB565 words: order them so that c0 >= c1 as uint16.  c0 == c1: every index 0, each texel's error its squared
 *   distance (over r, g, b) to the expanded c0.  Otherwise the four-colour palette of the decode rule above; each texel takes the
 *   palette entry of least squared distance, the lowest index on ties.  The block's error is the sum over its texels.
 *   Refine, at most three times: with the weights a = (3, 0, 2, 1)[index], b = 3 - a of the block's texels, Saa = sum(a a), Sbb =
 *   sum(b b), Sab = sum(a b), Sax_c = sum(a x_c), Sbx_c = sum(b x_c), det = Saa Sbb - Sab Sab.  det == 0: stop.  A_c = clamp((6 (Sbb
 *   Sax_c - Sab Sbx_c) + det) / (2 det), 0, 255), B_c = clamp((6 (Saa Sbx_c - Sab Sax_c) + det) / (2 det), 0, 255); quantise A and B
 *   and fit the pair: if its error is strictly smaller than the kept one it replaces c0, c1, the indices and the error, otherwise stop.
 *   Emit c0, c1 as little-endian uint16 and the sixteen indices in the bit order of the decode rule.  c0 >= c1 always, and with
 *   c0 == c1 only index 0 occurs: the three-colour mode's transparent index 3 is never emitted.
 * Parity with DirectXTex's mip filter and BC1 encoder (what the reference's import runs) is not pinned: neither is available. */
pbr_status pbr_bc1_encode(pbr_ctx* ctx, const void* texels, uint32_t width, uint32_t height, uint32_t mip_levels,
                          uint32_t stored_format, void* blocks_out);
/* The Use*Map flags of ConstantBufferInstance (gbuffer.hlsl:43-47) as texture indices, one record per draw in an array parallel
 * to the pbr_draw array: PBR_NO_MAP takes the constant branch, any other value is an index into the call's texture table. */
#define PBR_NO_MAP                   0xffffffffu
#define PBR_RASTER_MAX_TEXTURES      64u
typedef struct pbr_draw_maps {
    uint32_t albedo, normal, roughness, metallic, ao;
} pbr_draw_maps;
/* The sampler (SamplerLinearWrap, global.hlsli:21: MIN_MAG_MIP_LINEAR, wrap, MinLOD 0, MaxLOD FLT_MAX, no bias), pinned:
 *   Decode, before filtering: UNORM8 c -> c / 255 correctly rounded; the colour channels of _SRGB -> the sRGB curve of c / 255
 *   (x <= 0.04045 ? x / 12.92 : ((x + 0.055) / 1.055)^2.4) evaluated in double and rounded to fp32.  .x is red for every format
 *   (B8G8R8A8 swizzles); R8 reads as (r, 0, 0, 1).
 *   LOD, one per 2 x 2 quad and triangle: the quad origin (qx, qy) = (gx & ~1, gy & ~1) in global pixels; the winning
 *   triangle's perspective-correct uv at the pixel centres (qx + 1/2, qy + 1/2), (qx + 3/2, qy + 1/2), (qx + 1/2, qy + 3/2)
 *   gives ddx = uv10 - uv00, ddy = uv01 - uv00; per texture rho = max(|ddx * (w, h)|, |ddy * (w, h)|) (fp32, sqrtf), lambda =
 *   log2(rho) in double rounded to fp32 and clamped to [0, mip_levels - 1]; rho 0 or NaN gives lambda 0.
 *   Filter: l = floor(lambda), f = lambda - l; bilinear on levels l and min(l + 1, mip_levels - 1), blended by f.  Bilinear at
 *   texel coordinates (u w_l - 1/2, v h_l - 1/2): floor and fraction, both taps wrapped by non-negative modulo; each lerp is
 *   f == 0 ? a : fmaf(b, f, a (1 - f)) (x first, then y, then the levels), fp32 weights (not D3D's 8-bit fixed point). */
size_t pbr_gbuffer_raster_textured_scratch_bytes(uint32_t w, uint32_t h, uint32_t n_triangles);
size_t pbr_gbuffer_raster_textured_min_scratch_bytes(uint32_t w, uint32_t h, uint32_t n_triangles);
/* pbr_gbuffer_raster with maps != NULL: the pixel shader's map branches (gbuffer.hlsl:88-149), the same contract, plus
 *   maps: DEVICE array of n_draws records (the draw's maps); textures: HOST array of n_textures descriptors (copied by value).
 *   scratch is laid out, and its minimum sized, by the two _textured_ functions above.
 * Vertex stage adds tangent_ws = transpose(InvModel) (tangent, 0) (the normal's rule) and passes uv through; both are
 * interpolated perspective-correctly like the normal.  With a map: albedo = decode_gamma(sample.rgb); normal = normalize(ts.x t
 * + ts.y b + ts.z n) with n = normalize(normal_ws), t = normalize(tangent_ws), b = cross(n, t), ts = sample.rgb * 2 - 1;
 * roughness, metallic, AO = sample.x.  Without one: the constant (AO 0), bit-identical to the call with maps == NULL.
 * Guard on device data: a draw with a map index >= n_textures (other than PBR_NO_MAP) is dropped.
 * The table may mix decoded and BC1-resident textures (PBR_TEX_BC1_BLOCKS).  A BC1-resident texture samples exactly as the chain
 * pbr_bc1_decode produces from it (stored format = format & 0xff) would: the sampler reads each distinct block of a bilinear
 * footprint once (one 8-byte load), builds its palette once, picks the taps by their indices and then runs the same decode
 * tables, lerp order and LOD rule, so all five planes are bit-identical.  A table without a BC1 texture runs the kernel it ran
 * before the flag existed.
 * Refusals (PBR_ERR_INVALID, nothing enqueued): those of the call without maps; maps not 4-byte aligned; n_textures >
 * PBR_RASTER_MAX_TEXTURES, or textures null with n_textures > 0; a texture of another format (with PBR_TEX_BC1_BLOCKS: another
 * stored format), any other bit set in format, a zero size or one above PBR_TEX_MAX_SIZE, mip_levels 0 or above
 * floor(log2(min(w, h))) + 1, null or misaligned texels (BC1 blocks: 8 bytes); scratch below
 * pbr_gbuffer_raster_textured_min_scratch_bytes.  With maps == NULL (the constant-material raster): textures non-null or
 * n_textures != 0. */

/* ---- Model culling (new): Scene::CullModel + GBufferPass's mCullingStatus (DeferredPipeline.cpp:138-153) on the device ---------- */
/* A draw's bound in its local (vertex) space, 24 B; one per draw, parallel to the pbr_draw array. */
typedef struct pbr_aabb {
    float min[3], max[3];
} pbr_aabb;
/* mCullingStatus: draws_drawn = NumDrawCall, draws_culled = NumCulled; triangles_drawn = the triangles the call rasterizes (at most
 * max_triangles), triangles_culled = the sum of index_count / 3 over the culled draws (saturating at 2^32 - 1). */
typedef struct pbr_cull_stats {
    uint32_t draws_drawn, draws_culled, triangles_drawn, triangles_culled;
} pbr_cull_stats;
/* The bounds of each draw from the buffers the raster takes (the counterpart of the AABB the reference's mesh files carry):
 * out[d] = the exact min / max over the positions of the triangles of draw d, under the device-data guards of pbr_gbuffer_raster (a
 * range past n_indices is skipped whole; a triangle with an index + base_vertex outside [0, n_vertices) is dropped).  A draw with no
 * valid triangle gets the inverted box (min = +FLT_MAX, max = -FLT_MAX), which is never culled.  min / max are exact, so the result
 * is a function of the data alone.  vertices / indices / draws / out: DEVICE, 4-byte aligned.  One asynchronous launch on the
 * context's stream (one block per draw), no allocation.  Refusals (PBR_ERR_INVALID, nothing enqueued): a null or misaligned
 * pointer, a zero count, n_draws > PBR_RASTER_MAX_DRAWS. */
pbr_status pbr_draw_bounds(pbr_ctx* ctx, const pbr_vertex* vertices, uint32_t n_vertices, const uint32_t* indices, uint32_t n_indices,
                           const pbr_draw* draws, uint32_t n_draws, pbr_aabb* out);
/* pbr_gbuffer_raster with bounds != NULL, with or without maps: the model cull, the same contract, plus bounds (DEVICE, one
 * pbr_aabb per draw) and stats (DEVICE, may be NULL; written by the call's second launch).  A culled draw contributes no triangle:
 * it is neither set up nor binned.  max_triangles keeps its meaning (the sum over ALL draws); scratch sizes do not change.
 * The rule, pinned (tests/raster_cull_ref.py restates it; DESIGN.md derives it), fp32 unless stated, no contraction:
 *   World box of draw d (the box of all eight corners, centre / extent form; M = draws[d].Model):
 *     c = (min + max) * 0.5, e = (max - min) * 0.5
 *     cw_i = ((M[4i] c.x + M[4i+1] c.y) + M[4i+2] c.z) + M[4i+3],  ew_i = (|M[4i]| e.x + |M[4i+1]| e.y) + |M[4i+2]| e.z   (i = 0, 1, 2)
 *   Planes: six, in world space, formed on the host in fp64 from the fp32 g->Projection and g->View and rounded once to fp32.
 *     PV = Projection . View, each element ((p0 v0 + p1 v1) + p2 v2) + p3 v3, rows r0 .. r3.  The side planes are those of the TILE
 *     widened by one pixel on every side: xl = 2 (x0 - 1) / full_w - 1, xr = 2 (x0 + w + 1) / full_w - 1, yt = 1 - 2 (y0 - 1) / full_h,
 *     yb = 1 - 2 (y0 + h + 1) / full_h.  left r0 - xl r3, right xr r3 - r0, bottom r1 - yb r3, top yt r3 - r1, near r3 + r2 (the
 *     reference's, MathLib.h:1037; wider than the rasterizer's z >= 0), far r3 - r2.
 *   Test (FrustumVolume::Contains(AABB), MathLib.h:1057-1080, plus a slack), per plane p:
 *     d = ((p.x cw.x + p.y cw.y) + p.z cw.z) + p.w,  h = (|p.x ew.x| + |p.y ew.y|) + |p.z ew.z|,
 *     S = (((|p.x cw.x| + |p.y cw.y|) + |p.z cw.z|) + |p.w|) + h
 *     the draw is culled if and only if d < -(h + 2^-16 S) for some plane; a NaN anywhere keeps the draw.
 *   Never culled: a draw whose box is inverted (min > max on an axis) or not finite, or whose Model's last row is not exactly (0, 0, 0, 1).
 * Deviation from the reference: its AABB operator* (MathLib.cpp:5-10) transforms Min and Max only, which under-covers a rotated
 * model, and it culls against the whole frame's frustum.  Neither is copied.
 * THE INVARIANT: provided every vertex of every triangle of draw d lies in bounds[d] (pbr_draw_bounds gives such bounds), the five
 * planes are bit-identical to the same call without bounds, for every camera, tile, scratch size and texture format.
 * Refusals (PBR_ERR_INVALID, nothing enqueued): those of the call without bounds; bounds not 4-byte aligned; stats non-null and
 * not 4-byte aligned, or non-null while bounds is NULL.  Asynchronous: the same six launches, no host synchronisation, no allocation. */
/* The descriptor: 8-byte fields first, then the 32-bit ones (152 bytes, no padding), as pbr_shade_desc. */
typedef struct pbr_raster_desc {
    const pbr_global* g;
    const pbr_tile* tile;
    const pbr_vertex* vertices;
    const uint32_t* indices;
    const pbr_draw* draws;
    uint32_t* A;
    uint32_t* B;
    uint32_t* C;
    float* depth;
    uint8_t* stencil;
    void* scratch;
    size_t scratch_bytes;
    const pbr_draw_maps* maps;         /* maps, textures NULL and n_textures 0: the constant-material raster */
    const pbr_texture2d* textures;
    const pbr_aabb* bounds;            /* bounds, stats NULL: no model cull */
    pbr_cull_stats* stats;
    uint32_t n_vertices, n_indices, n_draws, max_triangles;
    uint32_t pitch;
    uint32_t n_textures;
} pbr_raster_desc;
pbr_status pbr_gbuffer_raster(pbr_ctx* ctx, const pbr_raster_desc* d);

/* ---- Depth-only rasterization (new): the depth plane of pbr_gbuffer_raster and nothing else ---------------------------------- */
/* What a shadow map or a depth pre-pass needs: 4 B per texel instead of the five planes' 17, and a scratch without the 80-byte
 * resolve record per triangle.  THE CONTRACT: for every input that pbr_gbuffer_raster accepts with maps == NULL, the depth plane
 * written here is BIT-IDENTICAL to the depth plane of that call — for every camera (perspective, or pbr_sun_fit's orthographic one),
 * every tile (own origin, ragged size, pitch > w), with or without bounds, and every scratch size from the minimum up; with bounds,
 * *stats is equal too.  Every pixel of the tile is written, 1.0 where nothing covers it; nothing outside the tile is touched.
 * There is no textured variant: gbuffer.hlsl has no clip / discard, so maps cannot change depth.
 * Why the bits agree: pbr_gbuffer_raster stores min(1, min over the covering fragments of z) — z is clamped to [0, 1], a NaN becomes
 * 0 and -0 never occurs, the plane starts at 1 and the test is LESS — a minimum over a totally ordered set, the same in any order.
 * This call shares the vertex stage, clip, snap, face test and bounding box with that call (one text), evaluates its coverage
 * and depth expressions per fragment and takes the minimum; it keeps no winner, counts no stencil, sorts no list, and walks a bin's
 * list whatever its length (the G-buffer call falls back to every triangle for a list of more than 2048).
 * Scratch: the G-buffer call's layout without the resolve records, so pbr_depth_raster_min_scratch_bytes(w, h, n) is at least 80 n
 * below pbr_gbuffer_raster_min_scratch_bytes(w, h, n); pbr_depth_raster_scratch_bytes is the recommended size (the same pool rule:
 * lists for about 8 bins per triangle).  Bins take list space in raster order until a list would end past the pool; that bin and
 * the bins after it have no list and walk every triangle record (which bins those are changes no bit).
 * Refusals (PBR_ERR_INVALID, nothing enqueued), those of pbr_gbuffer_raster: a null descriptor or pointer (bounds and stats may be
 * NULL), zero counts, n_draws > PBR_RASTER_MAX_DRAWS, max_triangles > PBR_RASTER_MAX_TRIANGLES, a bad tile, pitch < w, buffers not
 * 4-byte (scratch: 16-byte) aligned, stats without bounds, scratch below pbr_depth_raster_min_scratch_bytes(w, h, max_triangles);
 * and reserved != 0.  Asynchronous: six launches on the context's stream, no host synchronisation, no allocation. */
/* 8-byte fields first, then the 32-bit ones (104 bytes, no padding), as pbr_raster_desc. */
typedef struct pbr_depth_raster_desc {
    const pbr_global* g;
    const pbr_tile* tile;
    const pbr_vertex* vertices;
    const uint32_t* indices;
    const pbr_draw* draws;
    float* depth;
    void* scratch;
    size_t scratch_bytes;
    const pbr_aabb* bounds;            /* bounds, stats NULL: no model cull */
    pbr_cull_stats* stats;
    uint32_t n_vertices, n_indices, n_draws, max_triangles;
    uint32_t pitch;
    uint32_t reserved;                 /* must be 0 */
} pbr_depth_raster_desc;
pbr_status pbr_depth_raster(pbr_ctx* ctx, const pbr_depth_raster_desc* d);
size_t pbr_depth_raster_scratch_bytes(uint32_t w, uint32_t h, uint32_t n_triangles);
size_t pbr_depth_raster_min_scratch_bytes(uint32_t w, uint32_t h, uint32_t n_triangles);

/* bloom_prefilter.hlsl:17-60 (DeferredPipeline.cpp:411-427), ONE call described by a HOST struct (pointers first, then the 32-bit
 * fields: 64 bytes, no padding).  hdr: the w x h image, pitch `pitch` pixels.
 * rects == NULL and n_rects == 0: hdr -> out (w>>1 x h>>1), a dense plane; out_pitch, out_x and out_y must be 0.
 * Otherwise 1 .. 5 rectangles {x, y, w, h} of the half-res image (multi-GPU halo path): their texels are computed and stored at
 * out[(out_y + y) * out_pitch + (out_x + x)] — a tile writes the level-1 texels of its interior, or of the four bands of its border
 * ring in one launch, into the level-1 plane of its extended rectangle.  Texels outside the rectangles are left as they were.
 * Refusals (PBR_ERR_INVALID, nothing enqueued), in this order: a null descriptor; reserved != 0; hdr or out NULL ("null pointer");
 * rects NULL with n_rects != 0, rects with n_rects outside 1 .. 5 ("null pointer / 1 .. 5 rectangles"); no half-res texel, a side above
 * 65535, pitch < w ("bad size"); the dense form with out_pitch, out_x or out_y set; out_pitch or out_y above 65535 ("bad size"); then
 * the first faulty rectangle: "rect outside the half-res image", or "rect does not fit the output pitch" (out_pitch < out_x + x + w). */
typedef struct pbr_bloom_prefilter_desc {
    const pbr_half* hdr;
    pbr_half* out;
    const uint32_t (*rects)[4];
    uint32_t w, h, pitch;
    uint32_t out_pitch, out_x, out_y, n_rects;
    float threshold, knee;
    uint32_t reserved;                 /* must be 0 */
} pbr_bloom_prefilter_desc;
pbr_status pbr_bloom_prefilter(pbr_ctx* ctx, const pbr_bloom_prefilter_desc* d);
/* blur_horizontal.hlsl / blur.hlsli:24-55: in (iw x ih) sampled bilinearly at the texel
 * centres of out (ow x oh), 9 taps one OUTPUT texel apart in x. */
pbr_status pbr_blur_h(pbr_ctx* ctx, const pbr_half* in, uint32_t iw, uint32_t ih,
                      pbr_half* out, uint32_t ow, uint32_t oh);
/* blur_vertical.hlsl / blur.hlsli:58-89 */
pbr_status pbr_blur_v(pbr_ctx* ctx, const pbr_half* in, uint32_t iw, uint32_t ih,
                      pbr_half* out, uint32_t ow, uint32_t oh);
/* bloom_upsample_add.hlsl:13-25: out = H(lower) + H(upper), out has upper's size. */
pbr_status pbr_bloom_upsample_add(pbr_ctx* ctx, const pbr_half* upper, uint32_t uw, uint32_t uh,
                                  const pbr_half* lower, uint32_t lw, uint32_t lh, pbr_half* out);
/* bloom_merge.hlsl:7-11: hdr += in (both w x h; hdr pitch in pixels). */
pbr_status pbr_bloom_merge(pbr_ctx* ctx, pbr_half* hdr, uint32_t pitch, const pbr_half* in,
                           uint32_t w, uint32_t h);
/* One upsample level of BloomPass::Execute as ONE call (DeferredPipeline.cpp:472-540: the `Upsample Horizontal Add` +
 * `Blur Vertical` pair; with upper == NULL the `Upsample Merge` pair blur_horizontal + blur_vertical, :541-559, without the merge):
 *   out = V( H(upper) + H(lower sampled at out's size) )        out, upper: ow x oh;  lower: lw x lh, ow == 2 lw, oh == 2 lh
 * — the fused kernel pbr_bloom runs for such a level pair, exposed for stage-level tests and hosts that fuse the pair.  The H
 * result is rounded to fp16 where the first dispatch stores it.  Levels of >= 400 tiles of 128 x 32 texels take the polyphase
 * form of the 2x-up blur (csrc/bloom.hip: k_blur_up_poly): <= 1 fp16 ULP from the two staged calls (SURVEY 8c's bloom-stage
 * tolerance), not bit-identical; smaller levels are bit-identical.  Sizes must be even and <= 8192; out must not alias an input.
 * Alpha is taken as ONE constant per input plane (read at texel 0 of `lower` and of `upper`) and pushed through the same operations
 * once: every texel of an input must carry the same alpha — true of every level inside pbr_bloom, whose prefilter writes alpha 1. */
pbr_status pbr_bloom_up_level(pbr_ctx* ctx, const pbr_half* upper, const pbr_half* lower, uint32_t lw, uint32_t lh,
                              pbr_half* out, uint32_t ow, uint32_t oh);
/* BloomPass::Execute (DeferredPipeline.cpp:400-570), ONE call described by a HOST struct (pointers first, then the 32-bit fields: 88
 * bytes, no padding).  The rectangles are HOST arrays {x, y, w, h}.  chain_a / chain_b: pbr_bloom_chain_texels(w, h) half4 texels each
 * (BloomMipchain / BloomTempTexture) — SCRATCH: their contents after the call are unspecified.  (Wherever a level is exactly half the
 * one above and at most 8192 wide/high, the H and V pass of that level pair run as one kernel and the H result is never written;
 * elsewhere the staged kernels run.  Level 0 of chain_a — the V blur the merge consumes — is never written.)
 * WHOLE-IMAGE FORM, hdr_rect == NULL: all 16 dispatches on hdr, the w x h image (pitch hdr_pitch pixels).  hdr is bit-identical to
 * the sequence of stage calls above for frames below ~1.6 Mpixel; from there on the large 2x-up levels run in polyphase form
 * (pbr_bloom_up_level) and hdr is within 2 fp16 ULP of that sequence (>= 99.9 % of the texels identical).  hist_rect and hist256,
 * both set or both NULL: the luminance histogram (pbr_lum_histogram, min_log, inv_range) of hist_rect of the bloomed image, accumulated
 * inside the final bloom kernel (saves one full read of the HDR buffer); it ADDS into hist256 like the separate pass.
 * TILED FORM, hdr_rect != NULL: BloomPass::Execute minus its first dispatch, on the extended rectangle E (w x h, a multiple of 16 and
 * <= 8192 on a side) of a tile: level 1 of chain_a (offset pbr_bloom_level_offset(w, h, 1)) must hold the prefiltered image of ALL
 * of E — the interior from pbr_bloom_prefilter, the rest from the neighbouring tiles (pbr_halo_exchange); threshold and knee are
 * ignored.  Runs the 3 + 3 level pairs on E and merges (DeferredPipeline.cpp:521-570) only merge_rect of E into hdr, which covers
 * hdr_rect of E (hdr[0] = texel (hdr_rect.x, hdr_rect.y), pitch hdr_pitch pixels).  hist256 != NULL: the histogram of the merged
 * pixels is added.
 * Refusals (PBR_ERR_INVALID unless stated, nothing enqueued), in this order: a null descriptor; reserved != 0.  Whole-image form:
 * "merge_rect without hdr_rect"; "hist_rect without hist256" and "hist256 without hist_rect"; hist_rect empty or "rect outside the
 * image"; hdr or a chain NULL ("null pointer"); "image too small for 5 mips"; a side above 65535 or hdr_pitch < w ("bad size").
 * Tiled form: "hist_rect in the tiled form" (the histogram counts merge_rect); hdr, a chain or merge_rect NULL ("null pointer"); E too
 * small for 5 mips or above 65535 ("bad size"); "hdr_rect outside the extended tile" (or hdr_pitch below its width); "merge_rect
 * outside hdr_rect"; PBR_ERR_UNSUPPORTED for E odd or above 8192 on a side. */
typedef struct pbr_bloom_desc {
    pbr_half* hdr;
    pbr_half* chain_a;
    pbr_half* chain_b;
    uint32_t* hist256;
    const uint32_t* hdr_rect;          /* NULL: the whole-image form */
    const uint32_t* merge_rect;        /* tiled form only */
    const uint32_t* hist_rect;         /* whole-image form only */
    uint32_t w, h, hdr_pitch;
    float threshold, knee;
    float min_log, inv_range;
    uint32_t reserved;                 /* must be 0 */
} pbr_bloom_desc;
pbr_status pbr_bloom(pbr_ctx* ctx, const pbr_bloom_desc* d);

/* hdr_luminance_histogram.hlsl:23-59 (DeferredPipeline.cpp:276-298): ADDS into hist256. */
pbr_status pbr_lum_histogram(pbr_ctx* ctx, const pbr_half* hdr, uint32_t w, uint32_t h,
                             uint32_t pitch, float min_log, float inv_range, uint32_t* hist256);
/* hdr_average_histogram.hlsl:26-73 (DeferredPipeline.cpp:300-317): updates *avg_inout, zeroes hist. */
pbr_status pbr_lum_average(pbr_ctx* ctx, uint32_t* hist256, uint32_t pixel_count, float min_log,
                           float range, float delta_time, float* avg_inout);
/* hdr_tone_mapping.hlsl:9-52 (DeferredPipeline.cpp:320-336): hdr -> RGBA8 UNORM. */
pbr_status pbr_tonemap(pbr_ctx* ctx, const pbr_half* hdr, uint32_t w, uint32_t h, uint32_t pitch,
                       const float* avg, uint32_t* rgba8, uint32_t out_pitch);
/* hdr_average_histogram.hlsl + hdr_tone_mapping.hlsl as ONE launch (the last two dispatches of a frame): *avg_out = the adapted
 * luminance of pbr_lum_average(hist256, *avg_in), rgba8 = pbr_tonemap(hdr, *avg_out) — bit-identical to the two calls.  Every block of
 * the launch re-derives the average from the 256 bins, so NOTHING it reads may be written by it: avg_out != avg_in, and the histogram
 * zeroed "for the next frame" is hist_clear256 != hist256 (NULL: none) — a caller alternates two histograms (the next frame accumulates
 * into the one cleared here; the counts read here are cleared by the next frame's call) and two luminance cells. */
pbr_status pbr_average_tonemap(pbr_ctx* ctx, const uint32_t* hist256, uint32_t pixel_count, float min_log, float range, float delta_time,
                               const float* avg_in, float* avg_out, uint32_t* hist_clear256,
                               const pbr_half* hdr, uint32_t w, uint32_t h, uint32_t pitch, uint32_t* rgba8, uint32_t out_pitch);

/* ---- multi-view frames (new): N camera views of one scene per launch -------------------------------------------------- */
/* The reference renders one camera per FrameGraph; these entry points run the per-frame dispatches of up to PBR_MAX_VIEWS
 * equal-sized whole frames (w x h each, no tiles) as ONE launch chain (the view index in the grid; the average: one block per view).  Every view
 * gets exactly the bits its own single-view call would give: each kernel choice (exact-half vs staged bloom levels, polyphase
 * vs k_blur_hv, 16- vs 32-row tiles, staged cluster lists) follows one view's size, never the batch's.  Bloom levels that are
 * not an exact half (1920 x 1080 from level 3 down) run the staged single-view kernels once per view.
 * Shared by all views of a call: the size, the LUT, the padded env chain and the sky's SH pack (SkyBoxSH must be equal).
 * Errors (PBR_ERR_INVALID, nothing enqueued): n == 0 or n > PBR_MAX_VIEWS, a null pointer the call uses, SkyBoxSH that
 * differs between views, two views whose output buffers overlap, and every limit of the single-view call. */
#define PBR_MAX_VIEWS 16
typedef struct pbr_view {
    pbr_global       g;          /* camera, DeltaTime; SkyBoxSH must be the same in every view of a call */
    pbr_gbuffer      gb;         /* device planes of w x h pixels */
    const pbr_light* lights;     /* device, num_lights <= 1024 records; may alias another view's */
    int32_t          num_lights;
    pbr_cluster*     clusters;   /* device, PBR_NUM_CLUSTERS */
    pbr_half*        hdr;        /* device, w x h half4, pitch hdr_pitch pixels */
    uint32_t         hdr_pitch;
    pbr_half*        chain_a;    /* device, pbr_bloom_chain_texels(w, h) half4 each (scratch) */
    pbr_half*        chain_b;
    uint32_t*        hist256;    /* device, 256 bins */
    float*           avg;        /* device, the adapted-luminance cell */
    uint32_t*        rgba8;      /* device, w x h RGBA8, pitch out_pitch pixels */
    uint32_t         out_pitch;
} pbr_view;

/* ClusteredPass::Execute (DeferredPipeline.cpp:253-256) per view: pbr_clustered on every view (g, lights, num_lights, clusters). */
pbr_status pbr_clustered_views(pbr_ctx* ctx, const pbr_view* views, uint32_t n);
/* DeferredShadingPass::Execute (DeferredPipeline.cpp:187-206) per view: pbr_deferred_shade of the whole w x h frame
 * (g, gb, clusters, lights, num_lights -> hdr). */
pbr_status pbr_deferred_shade_views(pbr_ctx* ctx, const pbr_view* views, uint32_t n, uint32_t w, uint32_t h,
                                    const pbr_half* lut, uint32_t lut_res,
                                    const pbr_half* env_padded, uint32_t env_size, uint32_t env_mips);
/* BloomPass::Execute (DeferredPipeline.cpp:400-570) + the histogram dispatch (:276-298) per view: pbr_bloom's whole-image form with
 * the whole frame as hist_rect (hdr, chain_a, chain_b -> hist256, which it ADDS into). */
pbr_status pbr_bloom_histogram_views(pbr_ctx* ctx, const pbr_view* views, uint32_t n, uint32_t w, uint32_t h,
                                     float threshold, float knee, float min_log, float inv_range);
/* hdr_average_histogram.hlsl (DeferredPipeline.cpp:300-317) per view: pbr_lum_average(hist256, pixel_count, g.DeltaTime, avg). */
pbr_status pbr_lum_average_views(pbr_ctx* ctx, const pbr_view* views, uint32_t n, uint32_t pixel_count, float min_log, float range);
/* hdr_tone_mapping.hlsl (DeferredPipeline.cpp:320-336) per view: pbr_tonemap(hdr, avg -> rgba8) of the whole frame. */
pbr_status pbr_tonemap_views(pbr_ctx* ctx, const pbr_view* views, uint32_t n, uint32_t w, uint32_t h);

/* ---- multi-view sky resolve (new): the sky of N views per launch -------------------------------------------------------- */
/* SkyboxPass::Execute per view: pbr_skybox / pbr_skybox_bc6h of the whole w x h frame under views[v].g, on the pixels with
 * views[v].gb.stencil == 0 (pitch gb.pitch), into views[v].hdr (pitch hdr_pitch); the other fields of a view are not read and may be
 * null.  One launch (the view in the grid).  Every view's HDR target is bit-identical to its single-view call's; pixels with
 * stencil != 0 are untouched.  Refusals (PBR_ERR_INVALID, nothing enqueued): n == 0 or n > PBR_MAX_VIEWS, a null pointer the call
 * uses, a view's gb.pitch or hdr_pitch < w, two views whose HDR targets overlap, and every limit of the single-view call. */
pbr_status pbr_skybox_views(pbr_ctx* ctx, const pbr_view* views, uint32_t n, uint32_t w, uint32_t h, const pbr_cube_f32* sky);
pbr_status pbr_skybox_bc6h_views(pbr_ctx* ctx, const pbr_view* views, uint32_t n, uint32_t w, uint32_t h, const pbr_cube_bc6h* sky);

/* ---- Anti-aliasing (new): an edge filter on the tone-mapped RGBA8 target ------------------------------------------------------ */
/* The reference has no anti-aliasing of any kind, and the rasterizer resolves one sample per pixel: every silhouette is a staircase.
 * pbr_fxaa is a post-process filter of FXAA's structure (local-contrast test, edge orientation, a walk along the edge to its two ends,
 * a sub-pixel blend across it) under an all-integer rule that is this project's own, pinned here, restated in tests/fxaa_ref.py and
 * compiled for the host from the kernel's own text (csrc/fxaa_pixel.hpp, tools/fxaa_hostcheck.cpp).  The kernel is bit-identical to the
 * restatement on every pixel: nothing is floating point, so there is no tolerance.  It reads the RGBA8 image (R in the low byte) and
 * writes another one; it needs nothing from the G-buffer and sits after everything the reference defines.
 *
 * THE RULE.  Every read of a pixel outside [0, w) x [0, h) takes the nearest pixel inside (each coordinate clamped on its own).
 *   Luma        L = 77 R + 150 G + 29 B, an integer in 0 .. 65 280.
 *   Contrast    at pixel M with the 4-neighbours N, S, W, E (N is y - 1): hi, lo = max, min of the five lumas, range = hi - lo.
 *               range < max(4080, hi >> 3): M is not an edge pixel, its four bytes are copied.
 *   Orientation with the corners NW, NE, SW, SE:  eh = |NW + SW - 2W| + 2 |N + S - 2M| + |NE + SE - 2E|,
 *               ev = |NW + NE - 2N| + 2 |W + E - 2M| + |SW + SE - 2S|.  The edge is horizontal iff eh >= ev.  The pair across it is
 *               (a, b) = (N, S) for a horizontal edge, (W, E) for a vertical one; the walk runs along x resp. along y.
 *   Side        a if |a - M| >= |b - M|, else b.  nb = that neighbour, g = the larger absolute difference, P2 = L(M) + L(nb),
 *               m_lt = L(M) < L(nb).
 *   Walk        separately in the negative and the positive direction along the edge, over the offsets
 *               k = 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24 in that order:  e = L(m_k) + L(nb_k) - P2, m_k the pixel k steps
 *               along the edge from M (clamped), nb_k its neighbour on the chosen side (clamped).  Stop at the first k with
 *               2 |e| >= g; if none stops, keep k = 24 and that last e.  Results (kn, en) and (kp, ep).
 *   Edge offset kn < kp: dst = kn, good = (en < 0) != m_lt; otherwise dst = kp, good = (ep < 0) != m_lt.
 *               off8 = good ? 128 - (256 dst) / (kn + kp) : 0, the division floored.
 *   Sub-pixel   A = 2 (N + S + W + E) + NW + NE + SW + SE;  t = min(256, 256 |A - 12M| / (12 range)) floored;
 *               s = (t t (768 - 2t)) >> 16;  sub8 = (3 s s) >> 10, in 0 .. 192.
 *   Output      f8 = max(off8, sub8); R, G, B: out = (c_M (256 - f8) + c_nb f8 + 128) >> 8; alpha is M's, unchanged.
 * Choices the rule leaves to no one: ties go to "horizontal" (eh == ev), to side a (|a - M| == |b - M|) and to the positive walk
 * (kn == kp); g may be 0 (then both walks stop at k = 1); a pixel reads at most 24 pixels along one axis and 1 along the other.
 *
 * src, dst: device, 4-byte aligned, w x h pixels with pitches (in pixels) >= w; 16-byte accesses are used where a pointer and its
 * pitch are 16-byte multiples.  Refusals (PBR_ERR_INVALID, nothing enqueued): a null pointer, w or h of 0 (or above 65 535), a pitch
 * below w, and dst overlapping src: the filter cannot run in place. */
pbr_status pbr_fxaa(pbr_ctx* ctx, const uint32_t* src, uint32_t w, uint32_t h, uint32_t src_pitch, uint32_t* dst, uint32_t dst_pitch);
/* n <= PBR_MAX_VIEWS equal-sized images in ONE launch (the image index in the grid, the table by value in the kernel arguments):
 * each dst is bit-identical to its single call's.  Further refusals: n of 0 or above PBR_MAX_VIEWS, and any dst overlapping any
 * image's src or another dst (sources may alias each other). */
typedef struct pbr_fxaa_image {
    const uint32_t* src;
    uint32_t        src_pitch;
    uint32_t*       dst;
    uint32_t        dst_pitch;
} pbr_fxaa_image;
pbr_status pbr_fxaa_batch(pbr_ctx* ctx, const pbr_fxaa_image* images, uint32_t n, uint32_t w, uint32_t h);

/* ---- Sun light with a shadow map (new): a directional light added to the HDR target after the shade ---------------------------- */
/* The reference evaluates a directional light (deferred_shading.hlsl:144-156: dl_light_dir = normalize(1, 1, 1), 100 nits, through
 * brdf()) and never adds it, and it has no shadow code.  pbr_sun_light is that light as a pass of its own: it reads the
 * G-buffer the shade read, evaluates brdf() for one direction, looks the receiver up in a shadow map — the DEPTH PLANE of a
 * pbr_gbuffer_raster call under an orthographic light camera (pbr_sun_fit) — and adds the result to the fp16 HDR target, between the
 * shade (and the sky resolve) and the bloom.  pbr_depth_raster writes the same depth plane, bit for bit, without the A / B / C /
 * stencil planes the shadow pass otherwise writes and ignores (17 B per texel); the callers choose (DeferredFrame.set_sun(depth_only=),
 * pbrh_set_sun_shadow_depth_only).  Left out: multi-view frames, cascades, point-light shadows.
 *
 * THE RULE.  All arithmetic is fp32 with no contraction, in the order written (brackets first, otherwise left to right); every divide
 * and square root is the IEEE correctly rounded one — NO operation of this pass goes to the quick hardware units (v_rcp / v_rsq / v_log /
 * v_exp): its comparisons decide pixels, the pass is bound by its memory traffic, and tests/sun_truth.py restates it bit for bit.
 * Per pixel (x, y) of the tile with stencil > 0; every other pixel of hdr is untouched, bit for bit.  (gx, gy) = (x0 + x, y0 + y).
 *   Host, once per call: near_height = (float)(2.0 * (double)Near * tan((double)Fov / 2.0)), near_width = near_height * Ratio.
 *   (These are the shade's expressions for position_ws and view_ws, each operation IEEE: the shade itself takes near_height from the
 *   host's tanf, z_vs and 1 / Near from v_rcp and the camera vector from fused multiply-adds, so its receiver position may differ
 *   from this pass's in the last place or two — far inside either pass's tolerance, and of no consequence to the shadow test, which
 *   only this pass makes.)
 *   Material   albedo_c = byte_c(A) / 255 as byte * (1.0f / 255.0f) (c = r, g, b in bits 0-7, 8-15, 16-23; emission takes no part),
 *              roughness = byte0(C) * (1.0f / 255.0f), metallic = byte1(C) * (1.0f / 255.0f).
 *   Normal     e = (byte0(B), byte1(B)) * (1.0f / 255.0f); d = (e.x * 2 - 1, e.y * 2 - 1, 1 - |d.x| - |d.y|); if d.z < 0:
 *              (d.x, d.y) = (sign(d.x) * (1 - |d.y|), sign(d.y) * (1 - |d.x|)) from the old d.x, d.y, sign(0) = 1 (global.hlsli:85-115);
 *              N = d / sqrt(dot(d, d)), dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z.
 *   Position   u = (gx + 0.5) / full_w, v = (gy + 0.5) / full_h; cvv = ((2 u - 1) * 0.5 * near_width, (1 - 2 v) * 0.5 * near_height);
 *              camera_vec_i = (InvView[i][0] * cvv.x + InvView[i][1] * cvv.y) + InvView[i][2] * Near   (vs_main :91-121);
 *              z_vs = (Near * Far) / (Far - depth * (Far - Near)); position_ws = CameraPos + camera_vec * (z_vs / Near);
 *              w = CameraPos - position_ws; view_ws = w / sqrt(dot(w, w)).
 *   Radiance   L = Direction, NdotL = dot(N, L).  Not (NdotL > 0): the pixel is untouched and reads no shadow tap.
 *              Otherwise c = brdf * Luminance * NdotL per channel, brdf.hlsli:47-67 literally:
 *              h = L + view_ws; H = h / sqrt(dot(h, h)); NdotV = max(dot(N, view_ws), 0); NdotH = max(dot(N, H), 0);
 *              F0_c = 0.04 + (albedo_c - 0.04) * metallic; p = max(1 - NdotL, 1e-6); p5 = ((p * p) * (p * p)) * p (pow(p, 5) as
 *              multiplies); F_c = F0_c + (1 - F0_c) * p5; a = roughness * roughness; t = (NdotH * NdotH) * (a * a - 1) + 1;
 *              D = (a * a) / max((PI * t) * t, 1e-6); k = ((roughness + 1) * (roughness + 1)) * 0.125;
 *              G = (NdotV / max(NdotV * (1 - k) + k, 1e-6)) * (NdotL / max(NdotL * (1 - k) + k, 1e-6));
 *              Kd_c = (1 - F_c) * (1 - metallic); brdf_c = (Kd_c * albedo_c) * INV_PI + ((F_c * D) * G) / max((4 * NdotL) * NdotV, 0.0001);
 *              c_c = (brdf_c * Luminance_c) * NdotL.   PI = 3.14159265359f, INV_PI = 0.31830988618f (global.hlsli:4-7).
 *   Shadow     M = LightViewProj; q_i = ((M[i][0] * P.x + M[i][1] * P.y) + M[i][2] * P.z) + M[i][3], i = 0, 1, 2, P = position_ws;
 *              zr = q.z - (bias_const + bias_slope * (1 - NdotL));
 *              su = ((q.x + 1) * 0.5) * map_w - 0.5, sv = ((1 - q.y) * 0.5) * map_h - 0.5   (texel (ix, iy) has its centre at (ix, iy)).
 *   Taps       t(ix, iy) = 1 if (ix, iy) lies outside [0, map_w) x [0, map_h) or zr <= shadow_depth[iy * map_pitch + ix], else 0
 *              (a tie is lit: the map's own surface, stored with the same depth, is not shadowed by itself at zero bias).
 *              ix = floor(su), iy = floor(sv), wx = su - floor(su), wy = sv - floor(sv).
 *              B(i, j) = the bilinear footprint whose origin is texel (ix + i, iy + j), ALWAYS with the weights wx, wy of (su, sv):
 *              B = l(l(t00, t10, wx), l(t01, t11, wx), wy), l(a, b, w) = a + (b - a) * w, x first.
 *   Visibility shadow_depth == NULL: vis = 1.  A receiver with not (0 <= q.z <= 1), or with not (-2 <= su < map_w + 1 and
 *              -2 <= sv < map_h + 1) (every tap of either footprint set is then outside the map; NaN coordinates land here): vis = 1,
 *              no tap is read.  pcf == 1: vis = B(0, 0).  pcf == 3: vis = s * (1.0f / 9.0f), s = the sum of B(i, j) from 0 in the order
 *              j = -1, 0, 1 outer, i = -1, 0, 1 inner; the 4 x 4 taps are read once, lerped along x per tap row, then along y.
 *   Target     vis == 0: the pixel's bits are left alone.  Otherwise hdr.rgb = RN_half(float(hdr.rgb) + c * vis), the product rounded
 *              to fp32 before the sum; alpha's bits are kept.
 *   Probe      with contrib_f32 (float4 per pixel, tile-local, pitch hdr_pitch) EVERY pixel of the tile is written: (c * vis, 1) where
 *              stencil > 0 and NdotL > 0 (vis == 0 included), (0, 0, 0, 0) elsewhere; hdr must be NULL.
 * Direction must be finite and unit: |dot(d, d) - 1| <= 1e-4 in double.  LightViewProj must be affine: finite entries and row 3
 * exactly (0, 0, 0, 1).  Luminance and the biases must be finite.  g: InvView (its 3 x 3 part), CameraPos, Ratio, Near, Far, Fov are read
 * and must be finite (0 < Near < Far).
 * Refusals (PBR_ERR_INVALID, nothing enqueued): a null pointer (d, g, tile, gb, a G-buffer plane, sun); both or neither of hdr /
 * contrib_f32; an empty tile or one outside its frame; gb->pitch or hdr_pitch below the tile's width, map_pitch below map_w (with a
 * map); pcf not 1 or 3; the conditions on the sun above; with a map, map_w or map_h of 0 or above PBR_RASTER_MAX_SIZE; planes not
 * aligned to their element (hdr 8 bytes, contrib_f32 16, the rest 4); pitch x rows x 16 bytes (the G-buffer's and the target's) or
 * map_pitch x map_h x 4 bytes of 4 GiB or more (32-bit offsets, as for the shade); a non-finite camera.
 * ONE asynchronous launch on the context's stream, no allocation, no host synchronisation. */
typedef struct pbr_sun {            /* HOST struct */
    float Direction[3];             /* unit, world space, from the surface TOWARDS the light (dl_light_dir) */
    float Luminance[3];             /* light_luminance, deferred_shading.hlsl:146 */
    float LightViewProj[16];        /* world -> light clip, row-major, M*v; must be affine (row 3 == 0,0,0,1) */
    float bias_const, bias_slope;   /* in light-clip depth units */
    uint32_t pcf;                   /* 1 or 3 */
} pbr_sun;
typedef struct pbr_sun_desc {       /* pointers first, as pbr_shade_desc */
    const pbr_global* g; const pbr_tile* tile; const pbr_gbuffer* gb;
    const pbr_sun* sun;
    const float* shadow_depth;      /* map_w x map_h D32 plane: pbr_gbuffer_raster's depth plane or pbr_depth_raster's; NULL = no shadows */
    pbr_half* hdr;                  /* read-modify-write, tile-local, pitch hdr_pitch */
    float* contrib_f32;             /* parity probe: float4 per pixel, the contribution alone; exactly one of hdr / contrib_f32 */
    uint32_t map_w, map_h, map_pitch, hdr_pitch;
} pbr_sun_desc;
pbr_status pbr_sun_light(pbr_ctx* ctx, const pbr_sun_desc* d);
/* Host only, no ctx, no GPU: the light's pbr_global — View, InvView, Projection, InvProjection, Resolution; the rest zero — of an
 * orthographic light camera around a world-space box, and the matching LightViewProj.  The shadow pass is pbr_gbuffer_raster with
 * light_g, the tile {0, 0, map_w, map_h, map_w, map_h} and a scratch G-buffer of the map's size; its depth plane is the map.
 * THE RULE, in double unless stated, sums left to right; every matrix entry is rounded once to fp32:
 *   d = dir / |dir|.  z = -d (the light looks along -dir, left-handed like the reference's camera: +z into the scene);
 *   up = (0, 1, 0), or (1, 0, 0) when |d.y| > 0.999; x = cross(up, z) / |cross(up, z)|; y = cross(z, x).
 *   View = rows (x, 0), (y, 0), (z, 0), (0, 0, 0, 1) — the light's eye is the world origin, an orthographic camera has no position;
 *   InvView = its transpose.
 *   Extents: the min / max over the box's eight corners (each coordinate from min or max) of dot(x, p), dot(y, p), dot(z, p) ->
 *   l, r, b, t, n, f.  An extent below 1e-6 is replaced by 1e-6 about its centre.  x and y are widened by one texel of the FINAL map
 *   on each side: e = (r - l) / (map_w - 2), l -= e, r += e (y with map_h), so the corners lie within [-1 + 2 / map_w, 1 - 2 / map_w];
 *   z by 1 % of its span on each side: s = 0.01 * (f - n), n -= s, f += s, so the corners' depth lies within [0.01 / 1.02, 1.01 / 1.02].
 *   Projection (D3D orthographic, z in [0, 1]) = rows (2 / (r - l), 0, 0, -(r + l) / (r - l)), (0, 2 / (t - b), 0, -(t + b) / (t - b)),
 *   (0, 0, 1 / (f - n), -n / (f - n)), (0, 0, 0, 1); InvProjection = rows ((r - l) / 2, 0, 0, (r + l) / 2), (0, (t - b) / 2, 0,
 *   (t + b) / 2), (0, 0, f - n, n), (0, 0, 0, 1).  Resolution = (map_w, map_h).
 *   light_view_proj = the product, in double, of the fp32-ROUNDED Projection and View (what the raster's vertex stage multiplies by),
 *   rounded once; its row 3 is exactly (0, 0, 0, 1).
 * Refusals (PBR_ERR_INVALID): a null pointer, a non-finite or zero dir, a non-finite or inverted box (min > max), map_w or map_h
 * below 3 or above PBR_RASTER_MAX_SIZE. */
pbr_status pbr_sun_fit(const float dir[3], const pbr_aabb* world_box, uint32_t map_w, uint32_t map_h,
                       pbr_global* light_g, float light_view_proj[16]);

/* ---- multi-GPU (new) -------------------------------------------------------------- */
/* RCCL communicator over the ranks of one node.  unique_id: 128 bytes from
 * pbr_comm_unique_id() on rank 0, broadcast by the caller (e.g. torch.distributed store). */
pbr_status pbr_comm_unique_id(void* out_128_bytes);
/* Collective over all ranks.  Creates TWO communicators over the same ranks: the frame communicator (halo exchange)
 * from the unique id, and an ncclCommSplit of it for the histogram all-reduce — the two collectives may be in flight
 * on different streams at the same time (overlapped frame tail), and RCCL orders operations per communicator only. */
pbr_status pbr_comm_init(pbr_ctx* ctx, int world, int rank, const void* unique_id_128_bytes);
/* ncclAllReduce(sum, uint32, 256) on the ctx stream, on the histogram communicator; no-op without a communicator / world 1 */
pbr_status pbr_allreduce_hist(pbr_ctx* ctx, uint32_t* hist256);

/* Halo exchange of half4 rectangles of one plane (level 1 of the bloom pyramid) with neighbouring tiles: for every
 * peer, `send` = {x, y, w, h} of the plane that goes to rank `rank`, `recv` = the rectangle that arrives from it
 * (w == 0: nothing).  Both sides derive the rectangles from the tile layout, so sizes never travel.  One pack launch,
 * one ncclGroup of ncclSend / ncclRecv over xGMI, one unpack launch, all on the ctx stream.
 * staging: device scratch of pbr_halo_staging_bytes(); at most 16 peers. */
typedef struct pbr_halo_peer {
    int32_t  rank;
    uint32_t send[4];
    uint32_t recv[4];
} pbr_halo_peer;
size_t     pbr_halo_staging_bytes(const pbr_halo_peer* peers, uint32_t n_peers);
pbr_status pbr_halo_exchange(pbr_ctx* ctx, pbr_half* plane, uint32_t pitch, uint32_t rows,
                             const pbr_halo_peer* peers, uint32_t n_peers, void* staging, size_t staging_bytes);
/* the pack (unpack = 0: send rectangles -> staging) and unpack (unpack = 1: staging -> recv rectangles) halves on
 * their own, for a transport other than the context's communicator.  Staging layout: all send rectangles in peer
 * order, then all recv rectangles. */
pbr_status pbr_halo_pack(pbr_ctx* ctx, pbr_half* plane, uint32_t pitch, uint32_t rows,
                         const pbr_halo_peer* peers, uint32_t n_peers, void* staging, size_t staging_bytes, int unpack);

/* ---- measurement aid ---------------------------------------------------------------------------- */
/* Streaming read of `bytes` bytes (16-byte loads, grid-stride over `blocks` blocks of 256 lanes, one xor word per
 * block into sink[blocks]) on the ctx stream: the kernel bench.py times to report the MEASURED HBM-read bandwidth of
 * the device next to the 8 TB/s nominal peak.  buf 16-byte aligned. */
pbr_status pbr_membench_read(pbr_ctx* ctx, const void* buf, size_t bytes, uint32_t* sink, uint32_t blocks);
/* VALU issue-rate probe: `blocks` blocks of 256 lanes (one wave per SIMD each; blocks = CUs x waves-per-SIMD fills the
 * chip at that occupancy), every wave issuing iters x 8 independent instructions of one class — op 0: v_mul_f32 (the plain
 * class), 1: v_fma_f32, 2: v_pk_fma_f32 (packed fp32), 3: v_rcp_f32 (transcendental) — between two reads of the shader-core
 * cycle counter (s_memtime) and of the constant 100 MHz counter (s_memrealtime).  stamps: DEVICE, 4 x uint64 per wave
 * {cycles at start, at end, 100 MHz ticks at start, at end}, blocks * 4 waves.  With the launch duration (HIP events on the
 * ctx stream) this gives the chip's sustained issue rate in wave-instructions/s for that class AND the shader clock it holds
 * under that load — the denominators bench.py's `roofline.valu` needs from the box it runs on, not from a committed file. */
pbr_status pbr_valubench(pbr_ctx* ctx, uint32_t op, uint32_t blocks, uint32_t iters, uint64_t* stamps);

/* ---- Knobs build only (libpbr_hip_knobs.so, -DPBR_DEBUG_KNOBS): measurement entry points that are NOT part of the product library.
 * Round 6: the CU partition left the product API — measured in rounds 4-5 on four boxes it never paid (throughput mode with the
 * partition: +0 ... +8 % frame time; EXPERIMENTS.md), and a drop-in does not carry a switch nobody should flip. ---- */
#ifdef PBR_DEBUG_KNOBS
/* Partition the device's compute units between the context's private stream and its side stream (throughput mode: a frame's bloom +
 * exposure tail on the side stream's CUs while the next frame's shade has the others to itself — two kernels that both want the whole
 * chip only take turns otherwise).  masks: bit i = CU i (hipExtStreamCreateWithCUMask), `words` 32-bit words each; NULL = every CU.
 * On MI355X the bits run XCD by XCD in groups of four (bits 0-3 = four CUs of XCD 0, 4-7 = of XCD 1, ... 32-35 = the next four of XCD 0),
 * and a kernel's workgroups are dealt to the XCDs in equal shares whatever their CU counts: a partition must hold the same number of CUs
 * of every XCD, and a group of four bits is honoured as a whole only — i.e. a multiple of 32 low bits — or its XCD with the fewest sets the
 * pace (measured: profiles/r04_h_cu_partition_*.txt, r04_j_cu_partition_per_xcd.txt).
 * Masked streams are created with hipExtStreamCreateWithCUMask, which takes no flags: unlike the non-blocking streams they replace, they
 * SYNCHRONISE WITH THE LEGACY NULL STREAM — any null-stream work of the process (a hipMemset, a default-stream torch op or event record)
 * serialises both partitions, so no default-stream work belongs inside a partitioned frame.
 * Recreates both streams (the context must be idle on its private stream: pbr_ctx_use_own_stream, no side work pending) and
 * waits for the device.  A context bound to a foreign stream (pbr_ctx_set_stream) keeps that stream: only the side stream is masked. */
pbr_status  pbr_ctx_set_cu_masks(pbr_ctx* ctx, const uint32_t* main_mask, const uint32_t* side_mask, uint32_t words);
#endif

#ifdef __cplusplus
}
#endif
#endif /* PBR_HIP_H */
