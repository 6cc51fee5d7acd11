// tex_sampler.hpp — the textured resolve's sampler of pbr_gbuffer_raster: SamplerLinearWrap as pinned in include/pbr_hip.h (wrap
// addressing, bilinear taps, the quad's LOD, trilinear), on decoded textures and on BC1-resident ones read in place.  Included by
// gbuffer_raster.hip inside its anonymous namespace, after texel_decode.hpp (the decode tables the block stages into TexLds),
// bc1_decode.hpp (bc1_palette, bc1_texel) and tex_chain.hpp's tex2d::bc1_blocks; built with -ffp-contract=off like that file.
// tests/raster_tex_ref.py restates it in the same operation order; tests/sampler_truth.py holds it to an fp64 truth.
#pragma once

// the texture table and both decode tables, staged in LDS by the block
struct TexLds {
    pbr_texture2d tex[PBR_RASTER_MAX_TEXTURES];
    float dec[512];                        // [0, 256): kUnorm8, [256, 512): kSrgb8
};
__device__ __forceinline__ TexLds& tex_lds() {
    __shared__ TexLds tl;
    return tl;
}
// a texel coordinate's floor wrapped into [0, n) (non-negative modulo; fl is integral, so fmodf is exact)
__device__ __forceinline__ uint32_t wrap_texel(float fl, uint32_t n) {
    const float fn = (float)n;
    float m = fmodf(fl, fn);
    if (m < 0.0f) m += fn;
    return m >= 0.0f && m < fn ? (uint32_t)m : 0u;   // (a non-finite coordinate reads texel 0)
}
__device__ __forceinline__ float tex_lerp(float a, float b, float f) { return f == 0.0f ? a : fmaf(b, f, a * (1.0f - f)); }
// NC channels (.x, or .xyz) of texel i of a texture, decoded
template <int NC>
__device__ __forceinline__ void texel(const pbr_texture2d& t, const float* dec, size_t i, float* out) {
    if (t.format == PBR_TEX_R8_UNORM) {
        out[0] = dec[static_cast<const uint8_t*>(t.texels)[i]];
        if (NC == 3) { out[1] = 0.0f; out[2] = 0.0f; }
        return;
    }
    const uint32_t w = static_cast<const uint32_t*>(t.texels)[i];
    const float* tab = t.format == PBR_TEX_B8G8R8A8_UNORM_SRGB ? dec + 256 : dec;
    const uint32_t rs = t.format == PBR_TEX_R8G8B8A8_UNORM ? 0u : 16u;   // BGRA: red is byte 2, blue byte 0
    out[0] = tab[(w >> rs) & 255u];
    if (NC == 3) {
        out[1] = tab[(w >> 8) & 255u];
        out[2] = tab[(w >> (16u - rs)) & 255u];
    }
}
// a palette entry (bc1_decode.hpp: R | G << 8 | B << 16) of a BC1-resident texture, decoded as texel<NC> decodes the stored texel
template <int NC>
__device__ __forceinline__ void texel_rgba(uint32_t fmt, const float* dec, uint32_t w, float* out) {
    const float* tab = fmt == PBR_TEX_B8G8R8A8_UNORM_SRGB ? dec + 256 : dec;
    out[0] = tab[w & 255u];
    if (NC == 3) {
        const bool r8 = fmt == PBR_TEX_R8_UNORM;
        out[1] = r8 ? 0.0f : tab[(w >> 8) & 255u];
        out[2] = r8 ? 0.0f : tab[(w >> 16) & 255u];
    }
}
// the four taps of a BC1-resident level of bw x bh blocks at `blocks`: they lie in 1, 2 or 4 blocks; each distinct block is read
// once (8 bytes) and its palette built once
template <int NC>
__device__ __forceinline__ void taps_bc1(const uint2* blocks, uint32_t bw, uint32_t fmt, const float* dec, uint32_t x0, uint32_t y0,
                                         uint32_t x1, uint32_t y1, float* c00, float* c10, float* c01, float* c11) {
    const uint32_t bx0 = x0 >> 2, by0 = y0 >> 2, bx1 = x1 >> 2, by1 = y1 >> 2;
    const bool two_x = bx1 != bx0, two_y = by1 != by0;
    uint32_t pal[4], bits;
    auto fetch = [&](uint32_t bx, uint32_t by) {
        const uint2 b = blocks[(size_t)by * bw + bx];
        bc1_palette(b.x, pal);
        bits = b.y;
    };
    auto pick = [&](uint32_t x, uint32_t y) { return bc1_texel(pal, bits, x & 3u, y & 3u); };
    // every tap from the block of (x0, y0) first; a tap in another block is replaced when that block has been read
    fetch(bx0, by0);
    uint32_t w00 = pick(x0, y0), w10 = pick(x1, y0), w01 = pick(x0, y1), w11 = pick(x1, y1);
    if (two_x) {
        fetch(bx1, by0);
        w10 = pick(x1, y0);
        w11 = pick(x1, y1);
    }
    if (two_y) {
        fetch(bx0, by1);
        w01 = pick(x0, y1);
        w11 = pick(x1, y1);
        if (two_x) {
            fetch(bx1, by1);
            w11 = pick(x1, y1);
        }
    }
    texel_rgba<NC>(fmt, dec, w00, c00);
    texel_rgba<NC>(fmt, dec, w10, c10);
    texel_rgba<NC>(fmt, dec, w01, c01);
    texel_rgba<NC>(fmt, dec, w11, c11);
}
// bilinear on level l (wrap addressing).  BC1: the table may hold BC1-resident textures (the taps come from their blocks; the
// coordinates, the decode tables and the lerps are the same)
template <int NC, bool BC1>
__device__ __forceinline__ void bilinear(const pbr_texture2d& t, const float* dec, uint32_t l, float u, float v, float* out) {
    const bool blk = BC1 && (t.format & PBR_TEX_BC1_BLOCKS) != 0;
    size_t off = 0;                        // the level's first texel, or its first block
    for (uint32_t i = 0; i < l; i++)
        off += blk ? (size_t)bc1_blocks(t.width >> i) * bc1_blocks(t.height >> i) : (size_t)(t.width >> i) * (t.height >> i);
    const uint32_t wl = t.width >> l, hl = t.height >> l;
    const float x = u * (float)wl - 0.5f, y = v * (float)hl - 0.5f;
    const float flx = floorf(x), fly = floorf(y);
    const float fx = x - flx, fy = y - fly;
    const uint32_t x0 = wrap_texel(flx, wl), y0 = wrap_texel(fly, hl);
    const uint32_t x1 = x0 + 1u == wl ? 0u : x0 + 1u, y1 = y0 + 1u == hl ? 0u : y0 + 1u;
    float c00[NC], c10[NC], c01[NC], c11[NC];
    if (blk) {
        taps_bc1<NC>(static_cast<const uint2*>(t.texels) + off, bc1_blocks(wl), t.format & 0xffu, dec, x0, y0, x1, y1, c00, c10, c01, c11);
    } else {
        texel<NC>(t, dec, off + (size_t)y0 * wl + x0, c00);
        texel<NC>(t, dec, off + (size_t)y0 * wl + x1, c10);
        texel<NC>(t, dec, off + (size_t)y1 * wl + x0, c01);
        texel<NC>(t, dec, off + (size_t)y1 * wl + x1, c11);
    }
    for (int c = 0; c < NC; c++) out[c] = tex_lerp(tex_lerp(c00[c], c10[c], fx), tex_lerp(c01[c], c11[c], fx), fy);
}
// Sample(SamplerLinearWrap, uv) with the quad's uv differences (ddx, ddy): LOD, then trilinear
template <int NC, bool BC1>
__device__ __forceinline__ void sample(const pbr_texture2d& t, const float* dec, float u, float v, float dxu, float dxv, float dyu,
                                       float dyv, float* out) {
    const float fw = (float)t.width, fh = (float)t.height;
    const float ax = dxu * fw, ay = dxv * fh, bx = dyu * fw, by = dyv * fh;
    const float rho = fmaxf(sqrtf(ax * ax + ay * ay), sqrtf(bx * bx + by * by));
    float lam = rho > 0.0f ? (float)log2((double)rho) : 0.0f;            // 0 or NaN: 0
    lam = fminf(fmaxf(lam, 0.0f), (float)(t.mip_levels - 1u));
    const float fl = floorf(lam), f = lam - fl;
    const uint32_t l = (uint32_t)fl;
    bilinear<NC, BC1>(t, dec, l, u, v, out);
    if (f != 0.0f) {                       // (a level with weight 0 does not contribute: tex_lerp)
        float hi[NC];
        bilinear<NC, BC1>(t, dec, min(l + 1u, t.mip_levels - 1u), u, v, hi);
        for (int c = 0; c < NC; c++) out[c] = tex_lerp(out[c], hi[c], f);
    }
}
