// texture2d.hip — the chain of a 2D texture in both directions (include/pbr_hip.h, "Texture import" and PBR_TEX_BC1_BLOCKS).  The producing
// half is what the reference does when it imports an image (ResourceLoader::ImportTexture, ResourceLoader.cpp:252-277):
// GenerateImageMipmaps (:465-507) and TextureCompressor::Compress (TextureCompression.cpp:52-113, DirectX::Compress to BC1).
//   pbr_texture2d_gen_mips  the 2 x 2 box chain of a 2D texture in place, by the rule of scene.mip_chain.  k_tex_mips_tile: one block
//                           per 64 x 64 tile of level 0 takes it down levels 1 .. 6, each level's tile kept in LDS for the next
//                           (the 2 x 2 footprints are aligned at every level, so a tile never needs a neighbour's texels);
//                           k_tex_mips_top: one block makes levels 7 and up from level 6 (at most 128 x 128 texels), level after
//                           level through global memory.  Two launches instead of a last-block-done tail: no counter to zero, no
//                           cross-workgroup hand-off to get right, and the second launch is there only for chains above 7 levels.
//   pbr_bc1_encode          the inverse of pbr_bc1_decode: every level of a chain in one launch, lane = block.  The block's sixteen
//                           texels sit in sixteen registers as r | g << 8 | b << 16; each of its four rows is one 16-byte load
//                           (R8: 4 bytes), contiguous across the wave; no LDS and no cross-lane traffic.  The rule is pinned in the
//                           header, all in integers; tests/bc1_encode_ref.py restates it.
//   pbr_bc1_decode          the bulk decode of a whole BC1 chain, every level in one launch, lane = block (k_bc1_decode; the block
//                           rule is bc1_decode.hpp's, which the rasterizer's in-place sampler shares); pbr_texture2d_bytes beside it.
// Chain geometry — levels, offsets, block counts, refusals, the level table of the two lane = block kernels — is tex_chain.hpp's.
// Parity with DirectXTex's filter and encoder is not pinned (neither can run here): DESIGN.md section 7.
#include <cstdint>

#include "pbr_internal.hpp"
#include "tex_chain.hpp"
#include "bc1_decode.hpp"

namespace {

using tex2d::bc1_blocks;

// ---- pbr_texture2d_gen_mips ----
struct MipLevels {
    uint64_t first_texel[tex2d::MAX_LEVELS];   // the level's first texel in the chain
    uint32_t width, height, mips;
};
constexpr uint32_t MIP_TILE_LEVELS = 6;     // a 64 x 64 tile of level 0 ends in one texel of level 6

// (a + b + c + d + 2) >> 2 on each of the four bytes of a word: even and odd bytes in 16-bit fields (a field's sum is at most 1022)
__device__ __forceinline__ uint32_t avg4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    constexpr uint32_t M = 0x00ff00ffu;
    const uint32_t lo = (((a & M) + (b & M) + (c & M) + (d & M) + 0x00020002u) >> 2) & M;
    const uint32_t hi = ((((a >> 8) & M) + ((b >> 8) & M) + ((c >> 8) & M) + ((d >> 8) & M) + 0x00020002u) >> 2) & M;
    return lo | (hi << 8);
}
// a texel of TB bytes as a word (R8: the byte in bits 7-0, so avg4 serves both)
template <int TB>
__device__ __forceinline__ uint32_t load_texel(const uint8_t* p) {
    return TB == 4 ? *reinterpret_cast<const uint32_t*>(p) : (uint32_t)*p;
}
template <int TB>
__device__ __forceinline__ void store_texel(uint8_t* p, uint32_t v) {
    if (TB == 4) *reinterpret_cast<uint32_t*>(p) = v; else *p = (uint8_t)v;
}

// One block per 64 x 64 tile of level 0.  Level 1 (32 x 32 per tile): a thread makes four texels of one row from two rows of eight
// level-0 texels — 16-byte loads (R8: 8-byte), eight lanes on 256 contiguous bytes of a row — and stores them as one 16-byte word
// (R8: 4 bytes); rows that are not aligned to the vector and the tiles on the right / bottom edge go texel by texel.  Levels 2 .. 6
// come from the tile's previous level in LDS.  A texel of level l exists if x < width >> l and y < height >> l, and then so do the
// four above it, so the bounds test of each level's store is all the edge handling there is.
template <int TB>
__global__ __launch_bounds__(256) void k_tex_mips_tile(uint8_t* __restrict__ chain, MipLevels L) {
    __shared__ uint32_t tile[1024 + 256 + 64 + 16 + 4 + 1];
    const uint32_t t = threadIdx.x, tx = blockIdx.x, ty = blockIdx.y;
    constexpr uintptr_t LOAD_ALIGN = TB == 4 ? 15u : 7u, STORE_ALIGN = TB == 4 ? 15u : 3u;
    {
        const uint32_t w0 = L.width, w1 = L.width >> 1, h1 = L.height >> 1;
        const uint32_t lx = (t & 7u) * 4u, ly = t >> 3, x1 = tx * 32u + lx, y1 = ty * 32u + ly;
        uint32_t v[4] = {0u, 0u, 0u, 0u};
        if (x1 < w1 && y1 < h1) {
            const uint8_t* r0 = chain + ((uint64_t)(2u * y1) * w0 + 2u * x1) * TB;
            const uint8_t* r1 = r0 + (uint64_t)w0 * TB;
            const bool whole = x1 + 4u <= w1;
            uint32_t a[8], b[8];
            if (whole && (((uintptr_t)r0 | (uintptr_t)r1) & LOAD_ALIGN) == 0) {
                if (TB == 4) {
                    const uint4 a0 = reinterpret_cast<const uint4*>(r0)[0], a1 = reinterpret_cast<const uint4*>(r0)[1];
                    const uint4 b0 = reinterpret_cast<const uint4*>(r1)[0], b1 = reinterpret_cast<const uint4*>(r1)[1];
                    a[0] = a0.x; a[1] = a0.y; a[2] = a0.z; a[3] = a0.w; a[4] = a1.x; a[5] = a1.y; a[6] = a1.z; a[7] = a1.w;
                    b[0] = b0.x; b[1] = b0.y; b[2] = b0.z; b[3] = b0.w; b[4] = b1.x; b[5] = b1.y; b[6] = b1.z; b[7] = b1.w;
                } else {
                    const uint2 a0 = *reinterpret_cast<const uint2*>(r0), b0 = *reinterpret_cast<const uint2*>(r1);
                    for (uint32_t k = 0; k < 4u; k++) {
                        a[k] = (a0.x >> (8u * k)) & 255u; a[4u + k] = (a0.y >> (8u * k)) & 255u;
                        b[k] = (b0.x >> (8u * k)) & 255u; b[4u + k] = (b0.y >> (8u * k)) & 255u;
                    }
                }
            } else {
                for (uint32_t k = 0; k < 8u; k++) {
                    const bool in = 2u * x1 + k < 2u * w1;
                    a[k] = in ? load_texel<TB>(r0 + k * TB) : 0u;
                    b[k] = in ? load_texel<TB>(r1 + k * TB) : 0u;
                }
            }
            for (uint32_t k = 0; k < 4u; k++) v[k] = avg4(a[2u * k], a[2u * k + 1u], b[2u * k], b[2u * k + 1u]);
            uint8_t* dst = chain + (L.first_texel[1] + (uint64_t)y1 * w1 + x1) * TB;
            if (whole && ((uintptr_t)dst & STORE_ALIGN) == 0) {
                if (TB == 4) *reinterpret_cast<uint4*>(dst) = make_uint4(v[0], v[1], v[2], v[3]);
                else *reinterpret_cast<uint32_t*>(dst) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
            } else {
                for (uint32_t k = 0; k < 4u && x1 + k < w1; k++) store_texel<TB>(dst + k * TB, v[k]);
            }
        }
        for (uint32_t k = 0; k < 4u; k++) tile[ly * 32u + lx + k] = v[k];
    }
    uint32_t src = 0;                      // the previous level's tile in `tile`, n2 x n2 texels
    for (uint32_t l = 2, n2 = 32; l <= MIP_TILE_LEVELS && l < L.mips; l++, n2 >>= 1) {
        __syncthreads();
        const uint32_t n = n2 >> 1, dst = src + n2 * n2;
        if (t < n * n) {
            const uint32_t x = t % n, y = t / n;
            const uint32_t* s = tile + src + 2u * y * n2 + 2u * x;
            const uint32_t v = avg4(s[0], s[1], s[n2], s[n2 + 1u]);
            tile[dst + t] = v;
            const uint32_t wl = L.width >> l, hl = L.height >> l, gx = tx * n + x, gy = ty * n + y;
            if (gx < wl && gy < hl) store_texel<TB>(chain + (L.first_texel[l] + (uint64_t)gy * wl + gx) * TB, v);
        }
        src = dst;
    }
}

// One block: levels 7 .. mips - 1, each from the level above in global memory (level 7 is at most 128 x 128 texels).  The barrier
// between two levels orders the block's stores before its loads of them.
template <int TB>
__global__ __launch_bounds__(256) void k_tex_mips_top(uint8_t* chain, MipLevels L) {
    for (uint32_t l = MIP_TILE_LEVELS + 1u; l < L.mips; l++) {
        const uint32_t wl = L.width >> l, hl = L.height >> l, wp = L.width >> (l - 1u);
        const uint8_t* src = chain + L.first_texel[l - 1u] * TB;
        uint8_t* dst = chain + L.first_texel[l] * TB;
        for (uint32_t i = threadIdx.x; i < wl * hl; i += 256u) {
            const uint32_t x = i % wl, y = i / wl;
            const uint8_t* s = src + ((uint64_t)(2u * y) * wp + 2u * x) * TB;
            store_texel<TB>(dst + (uint64_t)i * TB, avg4(load_texel<TB>(s), load_texel<TB>(s + TB), load_texel<TB>(s + (uint64_t)wp * TB),
                                                        load_texel<TB>(s + ((uint64_t)wp + 1u) * TB)));
        }
        __syncthreads();
    }
}

// ---- pbr_bc1_encode ----
__device__ __forceinline__ int floor_div(int n, int d) {      // d > 0
    const int q = n / d;
    return (n < 0 && q * d != n) ? q - 1 : q;
}
__device__ __forceinline__ uint32_t quantise565(int r, int g, int b) {
    return (uint32_t)((((31 * r + 127) / 255) << 11) | (((63 * g + 127) / 255) << 5) | ((31 * b + 127) / 255));
}

// the fit of a pair of RGB565 words to the block (px: r | g << 8 | b << 16 per texel, valid: bit 4 y + x set for a texel of the level)
__device__ __forceinline__ void bc1_fit(const uint32_t (&px)[16], uint32_t valid, uint32_t ca, uint32_t cb, uint32_t& c0, uint32_t& c1,
                                        uint32_t& bits, uint32_t& err) {
    c0 = max(ca, cb);
    c1 = min(ca, cb);
    uint32_t pal[4];
    bc1_palette(c0 | (c1 << 16), pal);
    int pr[4], pg[4], pb[4];
    for (int k = 0; k < 4; k++) { pr[k] = pal[k] & 255u; pg[k] = (pal[k] >> 8) & 255u; pb[k] = (pal[k] >> 16) & 255u; }
    const bool one = c0 == c1;             // every index 0 (the palette of c0 <= c1 is the three-colour one: only entry 0 is used)
    bits = 0;
    err = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int r = px[i] & 255u, g = (px[i] >> 8) & 255u, b = (px[i] >> 16) & 255u;
        uint32_t d[4];
        for (int k = 0; k < 4; k++) d[k] = (uint32_t)((r - pr[k]) * (r - pr[k]) + (g - pg[k]) * (g - pg[k]) + (b - pb[k]) * (b - pb[k]));
        uint32_t best = d[0], idx = 0;
        if (!one) {
            if (d[1] < best) { best = d[1]; idx = 1; }
            if (d[2] < best) { best = d[2]; idx = 2; }
            if (d[3] < best) { best = d[3]; idx = 3; }
        }
        const bool in = (valid >> i) & 1u;
        bits |= in ? idx << (2 * i) : 0u;
        err += in ? best : 0u;
    }
}

// lane = block
__global__ __launch_bounds__(256) void k_bc1_encode(const uint8_t* __restrict__ texels, tex2d::Levels L, uint2* __restrict__ blocks) {
    const uint32_t bi = blockIdx.x * 256u + threadIdx.x;
    if (bi >= L.first_block[L.mips]) return;
    const uint32_t l = tex2d::level_of_block(L, bi);
    const uint32_t wl = L.width >> l, hl = L.height >> l, bw = bc1_blocks(wl);
    const uint32_t k = bi - L.first_block[l], bx = k % bw, by = k / bw;
    const uint32_t x0 = 4u * bx, y0 = 4u * by, nx = min(4u, wl - x0), ny = min(4u, hl - y0);

    uint32_t px[16], valid = 0;
#pragma unroll
    for (uint32_t y = 0; y < 4u; y++) {
        uint32_t s[4] = {0u, 0u, 0u, 0u};
        if (y < ny) {
            const uint8_t* row = texels + (L.first_texel[l] + (uint64_t)(y0 + y) * wl + x0) * L.texel_bytes;
            if (L.texel_bytes == 4u) {
                if (nx == 4u && ((uintptr_t)row & 15u) == 0) {
                    const uint4 q = *reinterpret_cast<const uint4*>(row);
                    s[0] = q.x; s[1] = q.y; s[2] = q.z; s[3] = q.w;
                } else {
                    for (uint32_t x = 0; x < 4u; x++) s[x] = x < nx ? reinterpret_cast<const uint32_t*>(row)[x] : 0u;
                }
                for (uint32_t x = 0; x < 4u; x++)
                    s[x] = L.bgra ? ((s[x] >> 16) & 255u) | (s[x] & 0xff00u) | ((s[x] & 255u) << 16) : s[x] & 0xffffffu;
            } else {
                if (nx == 4u && ((uintptr_t)row & 3u) == 0) {
                    const uint32_t q = *reinterpret_cast<const uint32_t*>(row);
                    for (uint32_t x = 0; x < 4u; x++) s[x] = (q >> (8u * x)) & 255u;
                } else {
                    for (uint32_t x = 0; x < 4u; x++) s[x] = x < nx ? (uint32_t)row[x] : 0u;
                }
                for (uint32_t x = 0; x < 4u; x++) s[x] *= 0x010101u;
            }
            valid |= ((1u << nx) - 1u) << (4u * y);
        }
        for (uint32_t x = 0; x < 4u; x++) px[4u * y + x] = s[x];
    }

    // start: the box's corners, paired per channel by the sign of its covariance with the channel of largest range
    const int n = __popc(valid);
    int lo[3] = {255, 255, 255}, hi[3] = {0, 0, 0}, sum[3] = {0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; i++) {
        if ((valid >> i) & 1u) {
            for (int c = 0; c < 3; c++) {
                const int x = (px[i] >> (8 * c)) & 255u;
                lo[c] = min(lo[c], x); hi[c] = max(hi[c], x); sum[c] += x;
            }
        }
    }
    int dom = 0;
    if (hi[1] - lo[1] > hi[dom] - lo[dom]) dom = 1;
    if (hi[2] - lo[2] > hi[dom] - lo[dom]) dom = 2;
    int sxd[3] = {0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; i++) {
        if ((valid >> i) & 1u) {
            const int xd = (px[i] >> (8 * dom)) & 255u;
            for (int c = 0; c < 3; c++) sxd[c] += (int)((px[i] >> (8 * c)) & 255u) * xd;
        }
    }
    const int sd = dom == 0 ? sum[0] : dom == 1 ? sum[1] : sum[2];
    int A[3], B[3];
    for (int c = 0; c < 3; c++) {
        const bool neg = n * sxd[c] - sum[c] * sd < 0;
        A[c] = neg ? lo[c] : hi[c];
        B[c] = neg ? hi[c] : lo[c];
    }
    uint32_t c0, c1, bits, err;
    bc1_fit(px, valid, quantise565(A[0], A[1], A[2]), quantise565(B[0], B[1], B[2]), c0, c1, bits, err);

    // refine: the least-squares endpoints of the current indices, kept while the error falls
    for (int it = 0; it < 3; it++) {
        int saa = 0, sbb = 0, sab = 0, sax[3] = {0, 0, 0}, sbx[3] = {0, 0, 0};
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if ((valid >> i) & 1u) {
                const int a = (0x1203 >> (4 * ((bits >> (2 * i)) & 3u))) & 3, b = 3 - a;
                saa += a * a; sbb += b * b; sab += a * b;
                for (int c = 0; c < 3; c++) {
                    const int x = (px[i] >> (8 * c)) & 255u;
                    sax[c] += a * x; sbx[c] += b * x;
                }
            }
        }
        const int det = saa * sbb - sab * sab;
        if (det == 0) break;
        for (int c = 0; c < 3; c++) {
            A[c] = min(max(floor_div(6 * (sbb * sax[c] - sab * sbx[c]) + det, 2 * det), 0), 255);
            B[c] = min(max(floor_div(6 * (saa * sbx[c] - sab * sax[c]) + det, 2 * det), 0), 255);
        }
        uint32_t n0, n1, nbits, nerr;
        bc1_fit(px, valid, quantise565(A[0], A[1], A[2]), quantise565(B[0], B[1], B[2]), n0, n1, nbits, nerr);
        if (nerr >= err) break;
        c0 = n0; c1 = n1; bits = nbits; err = nerr;
    }
    blocks[bi] = make_uint2(c0 | (c1 << 16), bits);
}

// ---- pbr_bc1_decode: every level of a chain in one launch ----
// lane = block: its palette once, then its rows.  A row that lies whole inside the level and is aligned to its own size is one
// vector store (16 bytes, R8: 4); the rows of edge blocks of sizes that are no multiple of 4, and unaligned ones, go texel by texel.
__global__ __launch_bounds__(256) void k_bc1_decode(const uint2* __restrict__ blocks, tex2d::Levels L, uint8_t* __restrict__ out) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= L.first_block[L.mips]) return;
    const uint32_t l = tex2d::level_of_block(L, b);
    const uint32_t wl = L.width >> l, hl = L.height >> l, bw = bc1_blocks(wl);
    const uint32_t k = b - L.first_block[l], bx = k % bw, by = k / bw;
    const uint2 blk = blocks[b];
    uint32_t pal[4];
    bc1_palette(blk.x, pal);
    const uint32_t x0 = 4u * bx, nx = min(4u, wl - x0);
    for (uint32_t y = 0; y < 4u && 4u * by + y < hl; y++) {
        uint32_t px[4];
        for (uint32_t x = 0; x < 4u; x++) px[x] = bc1_texel(pal, blk.y, x, y);
        uint8_t* row = out + (L.first_texel[l] + (uint64_t)(4u * by + y) * wl + x0) * L.texel_bytes;
        if (L.texel_bytes == 4u) {
            for (uint32_t x = 0; x < 4u; x++) px[x] = bc1_stored(px[x], L.bgra != 0);
            if (nx == 4u && ((uintptr_t)row & 15u) == 0) {
                *reinterpret_cast<uint4*>(row) = make_uint4(px[0], px[1], px[2], px[3]);
            } else {
                for (uint32_t x = 0; x < nx; x++) reinterpret_cast<uint32_t*>(row)[x] = px[x];
            }
        } else {
            if (nx == 4u && ((uintptr_t)row & 3u) == 0) {
                *reinterpret_cast<uint32_t*>(row) = (px[0] & 255u) | ((px[1] & 255u) << 8) | ((px[2] & 255u) << 16) | (px[3] << 24);
            } else {
                for (uint32_t x = 0; x < nx; x++) row[x] = (uint8_t)px[x];
            }
        }
    }
}

}  // namespace

extern "C" {

pbr_status pbr_texture2d_gen_mips(pbr_ctx* ctx, void* texels, uint32_t width, uint32_t height, uint32_t mip_levels, uint32_t format) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, texels, "pbr_texture2d_gen_mips: null pointer");
    PBR_CHECK(ctx, "pbr_texture2d_gen_mips", tex2d::refusal(width, height, mip_levels, format));
    PBR_REQUIRE(ctx, tex2d::aligned(texels, format), "pbr_texture2d_gen_mips: texels not aligned to the texel size");
    if (mip_levels == 1) return PBR_OK;
    tex2d::Levels T;
    tex2d::fill(T, width, height, mip_levels, format);
    MipLevels L;                           // (the texel half of the table: its kernels' argument keeps its layout)
    L.width = width; L.height = height; L.mips = mip_levels;
    for (uint32_t l = 0; l < tex2d::MAX_LEVELS; l++) L.first_texel[l] = T.first_texel[l];
    uint8_t* chain = static_cast<uint8_t*>(texels);
    const dim3 grid((width + 63u) / 64u, (height + 63u) / 64u);
    if (format == PBR_TEX_R8_UNORM) hipLaunchKernelGGL(k_tex_mips_tile<1>, grid, dim3(256), 0, ctx->stream, chain, L);
    else hipLaunchKernelGGL(k_tex_mips_tile<4>, grid, dim3(256), 0, ctx->stream, chain, L);
    if (pbr_status st = pbr::launched(ctx, "k_tex_mips_tile")) return st;
    if (mip_levels > MIP_TILE_LEVELS + 1u) {
        if (format == PBR_TEX_R8_UNORM) hipLaunchKernelGGL(k_tex_mips_top<1>, dim3(1), dim3(256), 0, ctx->stream, chain, L);
        else hipLaunchKernelGGL(k_tex_mips_top<4>, dim3(1), dim3(256), 0, ctx->stream, chain, L);
        return pbr::launched(ctx, "k_tex_mips_top");
    }
    return PBR_OK;
}

pbr_status pbr_bc1_encode(pbr_ctx* ctx, const void* texels, uint32_t width, uint32_t height, uint32_t mip_levels,
                          uint32_t stored, void* blocks_out) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, texels && blocks_out, "pbr_bc1_encode: null pointer");
    PBR_CHECK(ctx, "pbr_bc1_encode", tex2d::refusal(width, height, mip_levels, stored));
    PBR_REQUIRE(ctx, tex2d::aligned(blocks_out, PBR_TEX_BC1_BLOCKS) && tex2d::aligned(texels, stored),
                "pbr_bc1_encode: blocks_out not 8-byte aligned, or texels not aligned to the texel size");
    tex2d::Levels L;
    tex2d::fill(L, width, height, mip_levels, stored);
    const uint32_t nb = L.first_block[mip_levels];
    hipLaunchKernelGGL(k_bc1_encode, dim3((nb + 255u) / 256u), dim3(256), 0, ctx->stream, static_cast<const uint8_t*>(texels), L,
                       static_cast<uint2*>(blocks_out));
    return pbr::launched(ctx, "k_bc1_encode");
}

size_t pbr_texture2d_bytes(uint32_t width, uint32_t height, uint32_t mip_levels, uint32_t format) {
    return tex2d::chain_bytes(width, height, mip_levels, format);
}

pbr_status pbr_bc1_decode(pbr_ctx* ctx, const void* blocks, uint32_t width, uint32_t height, uint32_t mip_levels,
                          uint32_t stored, void* out) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, blocks && out, "pbr_bc1_decode: null pointer");
    PBR_CHECK(ctx, "pbr_bc1_decode", tex2d::refusal(width, height, mip_levels, stored));
    PBR_REQUIRE(ctx, tex2d::aligned(blocks, PBR_TEX_BC1_BLOCKS) && tex2d::aligned(out, stored),
                "pbr_bc1_decode: blocks not 8-byte aligned, or out not aligned to the texel size");
    tex2d::Levels L;
    tex2d::fill(L, width, height, mip_levels, stored);
    const uint32_t nb = L.first_block[mip_levels];
    hipLaunchKernelGGL(k_bc1_decode, dim3((nb + 255u) / 256u), dim3(256), 0, ctx->stream, static_cast<const uint2*>(blocks), L,
                       static_cast<uint8_t*>(out));
    return pbr::launched(ctx, "k_bc1_decode");
}

}  // extern "C"
