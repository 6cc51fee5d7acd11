// bloom.hip — bloom chain on gfx950: soft-knee prefilter, separable 9-tap Gaussian pyramid, upsample-add and merge
// (bloom_prefilter.hlsl, blur.hlsli, blur_horizontal/vertical.hlsl, bloom_upsample_add.hlsl, bloom_merge.hlsl; schedule
// BloomPass::Execute, DeferredPipeline.cpp:400-570).  Compiled with -ffp-contract=off and written in the oracle's operation order
// (fused multiply-adds only where the oracle writes fmaf: sampler lerps and the blur's multiply-accumulate), so every stage is
// bit-identical to the CPU oracle on the same input; k_blur_up_poly alone is ULP-bounded (see there).
//
// Map of the file:
//  1. STAGED kernels, one per reference dispatch, any image size (k_bloom_prefilter, k_blur_h, k_blur_v, k_bloom_merge), and
//     k_blur_v_merge = the last V pass + merge + histogram.  H passes keep the reference's 256-texel row groups with the sampled
//     row in LDS like blur.hlsli's Cache[]; V passes use 64 x 16 tiles staged through LDS (vtile_*), not the reference's 1 x 256
//     column groups (one texel per 8 KiB-strided row), so that global accesses stay 512-byte coalesced.
//  2. Pieces the merging kernels share: luminance bin, per-wave histograms (hist_*), the merge rounding (merge_rounded*).
//  3. FUSED kernels for exact 2x pyramids, bit-identical to the staged ones: k_bloom_prefilter_2x (shared samples), k_blur_hv
//     (H + V of a level [+ merge + histogram] on a tile) and k_blur_up_poly (large 2x-up levels), with what those two share:
//     TailRect and its tests, level_args (view selection), level_alpha, wave_sync; and k_bloom_small_end, which computes pyramid
//     levels 4 and 3 inside level 2's up-pass launch (per tile, in LDS, on the region the tile taps) in k_blur_hv's operation order.
//  4. Launch: tail_rect / tile_grid / launch_hv (the fused kernels' choice), prefilter_launch, the checks entry points share.
//  5. C ABI of the staged passes; the schedule (bloom_pass, up_pass_rects; when the small end is folded: there); C ABI of the chain.
#include <type_traits>
#include "pbr_internal.hpp"
#include "pbr_device.hpp"

using namespace pbr;

__constant__ float c_gauss[9] = {0.0148f, 0.0459f, 0.1050f, 0.1941f, 0.2803f, 0.1941f, 0.1050f, 0.0459f, 0.0148f};   // blur.hlsli:17

__device__ __forceinline__ float4 to4(F4 v) { return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ F4 from4(float4 v) { return f4(v.x, v.y, v.z, v.w); }

// ---------------------------------------------------------------- bloom_prefilter.hlsl:17-60
// grid (ceil(ow/64), ceil(oh/4)), block (64,4): one thread per half-res texel
// OutRect: the outputs [x0,x1) x [y0,y1) (half-res texels of this image) are computed and stored at
// out[(y + oy) * out_pitch + (x + ox)] — the whole image into a dense plane is {0,0,ow,oh}, pitch ow, offset 0;
// a tile's interior into the level-1 plane of its extended rectangle is the multi-GPU halo path.
struct OutRect { int x0, y0, x1, y1, ox, oy, pitch; };
// several output rectangles in one launch of the shared-sample kernel (1-D grid; the overlapped multi-GPU frame
// prefilters the four bands of its border ring at once): rectangle r owns blocks first[r] .. first[r+1]-1
constexpr int PF_MAX_RECTS = 5;
struct OutRects {
    int n, ox, oy, pitch;
    int x0[PF_MAX_RECTS], y0[PF_MAX_RECTS], x1[PF_MAX_RECTS], y1[PF_MAX_RECTS], tiles_x[PF_MAX_RECTS], first[PF_MAX_RECTS + 1];
};
// bloom_prefilter.hlsl:36-47 — one bilinear sample c through the soft knee (its three IEEE divides): (colour x weight, weight)
__device__ __forceinline__ float4 soft_knee_sample(F4 c, float threshold, float knee) {
    const float brightness = fmaxf(c.x, fmaxf(c.y, c.z));
    float soft = fminf(fmaxf(brightness - threshold + threshold * knee, 0.0f), 2.0f * threshold * knee);
    soft /= 4.0f * threshold * knee + 0.00001f;
    const float contribution = fmaxf(soft, brightness - threshold) / fmaxf(brightness, 0.00001f);
    const float cr = c.x * contribution, cg = c.y * contribution, cb = c.z * contribution;
    const float wgt = 1.0f / (luminance(cr, cg, cb) + 1.0f);
    return make_float4(cr * wgt, cg * wgt, cb * wgt, wgt);
}

__global__ __launch_bounds__(256) void k_bloom_prefilter(const pbr_half* __restrict__ hdr, int w, int h, int pitch,
                                                           pbr_half* __restrict__ out, OutRect rc,
                                                           float tx, float ty, float threshold, float knee) {
    const int x = rc.x0 + blockIdx.x * 64 + threadIdx.x;
    const int y = rc.y0 + blockIdx.y * 4 + threadIdx.y;
    if (x >= rc.x1 || y >= rc.y1) return;
    const float u = (float)x * tx, v = (float)y * ty;   // no +0.5 (Q9)
    const float ox[5] = {0.0f, -1.0f, -1.0f, 1.0f, 1.0f};
    const float oy[5] = {0.0f, -1.0f, 1.0f, -1.0f, 1.0f};
    float tr = 0.0f, tg = 0.0f, tb = 0.0f, tw = 0.0f;
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const float4 s = soft_knee_sample(sample_2d_h4(hdr, w, h, pitch, u + ox[i] * tx, v + oy[i] * ty), threshold, knee);
        tr += s.x; tg += s.y; tb += s.z;
        tw += s.w;
    }
    if (tw > 0.0f) { tr /= tw; tg /= tw; tb /= tw; }
    store_h4(out + 4 * ((size_t)(y + rc.oy) * rc.pitch + (x + rc.ox)), f4(tr, tg, tb, 1.0f));
}

// ---------------------------------------------------------------- blur.hlsli:24-55
// One 256-thread group = 256 consecutive output texels of a row, the bilinear-sampled row cached in LDS
// (264 float4 entries incl. the 4+4 halo slots) exactly like the shader's Cache[].  A block walks HB_ROWS
// rows of its column group and software-pipelines them: the four raw taps of row r+1 are in flight while
// row r is filtered out of a double-buffered cache (one barrier per row); a one-row block is latency-bound.
constexpr int HB_MAX_ROWS = 8;   // rows per block: chosen per launch so that small pyramid levels still fill the chip
struct RawTap {   // the four texels of one bilinear sample, still in half precision, + the y weight
    H4 c00, c10, c01, c11;
    float fy;
};
struct ColumnCoord { int x0, x1; float fx; };   // x side of a sample: row-invariant
__device__ __forceinline__ ColumnCoord column_coord(float u, int iw) {
    const BilinearCoord c = bilinear_coord(u, iw);
    return ColumnCoord{clampi(c.i0, 0, iw - 1), clampi(c.i1, 0, iw - 1), c.f};
}
__device__ __forceinline__ RawTap load_tap(const pbr_half* __restrict__ in, int iw, int ih, const ColumnCoord& cc, float v) {
    const BilinearCoord cy = bilinear_coord(v, ih);
    const int y0 = clampi(cy.i0, 0, ih - 1), y1 = clampi(cy.i1, 0, ih - 1);
    const H4* r0 = reinterpret_cast<const H4*>(in) + (size_t)y0 * iw;
    const H4* r1 = reinterpret_cast<const H4*>(in) + (size_t)y1 * iw;
    return RawTap{r0[cc.x0], r0[cc.x1], r1[cc.x0], r1[cc.x1], cy.f};
}
__device__ __forceinline__ F4 h4f(H4 h) { return f4((float)h.x, (float)h.y, (float)h.z, (float)h.w); }
__device__ __forceinline__ float4 finish_tap(const RawTap& r, float fx) {
    return to4(bilerp(h4f(r.c00), h4f(r.c10), h4f(r.c01), h4f(r.c11), fx, r.fy));
}
__device__ __forceinline__ F4 gauss9(const float4* c) {
    F4 v = f4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int i = 0; i < 9; i++) v = fma4(from4(c[i]), c_gauss[i], v);   // value += pixel * weight (fused mad)
    return v;
}

// grid (ceil(ow/256), ceil(oh/rows_per_block)), block 256.  DUAL: bloom_upsample_add.hlsl:13-25 (lower first, then upper)
template <bool DUAL>
__global__ __launch_bounds__(256) void k_blur_h(const pbr_half* __restrict__ in, int iw, int ih,
                                                 const pbr_half* __restrict__ in2, int iw2, int ih2,
                                                 pbr_half* __restrict__ out, int ow, int oh, float tx, float ty, int rows_per_block) {
    constexpr int NS = DUAL ? 2 : 1;
    __shared__ float4 cache[2][NS][264];
    const int t = threadIdx.x;
    const int gx0 = blockIdx.x * 256;
    const int y_begin = blockIdx.y * rows_per_block, y_end = min(y_begin + rows_per_block, oh);
    // sample positions in x (blur.hlsli:26-43): every thread its own texel; threads 0-3 / 252-255 also one halo tap
    const float uvx = ((float)(gx0 + t) + 0.5f) * tx;
    const bool halo = (t < 4) | (t >= 252);
    const float uvx_h = t < 4 ? fmaxf(uvx - 4.0f * tx, 0.0f) : fminf(uvx + 4.0f * tx, 1.0f);
    const int slot_h = t < 4 ? t : t + 8;
    const ColumnCoord cm = column_coord(uvx, iw), ch = column_coord(uvx_h, iw);
    ColumnCoord cm2 = cm, ch2 = ch;
    if (DUAL) { cm2 = column_coord(uvx, iw2); ch2 = column_coord(uvx_h, iw2); }

    RawTap m[NS], hh[NS];
    auto load_row = [&](int y) {
        const float uvy = ((float)y + 0.5f) * ty;
        m[0] = load_tap(in, iw, ih, cm, uvy);
        if (halo) hh[0] = load_tap(in, iw, ih, ch, uvy);
        if (DUAL) {
            m[NS - 1] = load_tap(in2, iw2, ih2, cm2, uvy);
            if (halo) hh[NS - 1] = load_tap(in2, iw2, ih2, ch2, uvy);
        }
    };
    load_row(y_begin);
    for (int y = y_begin; y < y_end; y++) {
        const int buf = (y - y_begin) & 1;
        cache[buf][0][t + 4] = finish_tap(m[0], cm.fx);
        if (halo) cache[buf][0][slot_h] = finish_tap(hh[0], ch.fx);
        if (DUAL) {
            cache[buf][NS - 1][t + 4] = finish_tap(m[NS - 1], cm2.fx);
            if (halo) cache[buf][NS - 1][slot_h] = finish_tap(hh[NS - 1], ch2.fx);
        }
        __syncthreads();
        if (y + 1 < y_end) load_row(y + 1);   // in flight while this row is filtered
        const int x = gx0 + t;
        if (x < ow) {
            F4 v = gauss9(cache[buf][0] + t);
            if (DUAL) v = v + gauss9(cache[buf][NS - 1] + t);
            store_h4(out + 4 * ((size_t)y * ow + x), v);
        }
    }
}

// ---------------------------------------------------------------- blur.hlsli:58-89
// 64 x 16 output tiles; TR divides 256 so a tile never straddles one of the reference's
// 256-row groups, which decides whether a halo row uses the group-edge position formula.
constexpr int VT_W = 64, VT_R = 16;
// the tile's VT_R + 8 sampled rows y0 - 4 .. y0 + VT_R + 3 at column x into LDS (block (VT_W, 4): thread row threadIdx.y takes every fourth)
__device__ __forceinline__ void vtile_sample(float4 (*smp)[VT_W], const pbr_half* __restrict__ in, int iw, int ih, int x, int y0, float tx, float ty) {
    const bool top_edge = (y0 & 255) == 0;
    const bool bot_edge = ((y0 + VT_R) & 255) == 0;
    const float uvx = ((float)x + 0.5f) * tx;
    for (int r = threadIdx.y; r < VT_R + 8; r += 4) {
        const int j = y0 - 4 + r;   // sampled row (may be outside the image)
        float vy;
        if (r < 4 && top_edge) vy = fmaxf(((float)(j + 4) + 0.5f) * ty - 4.0f * ty, 0.0f);                  // Cache[gtid.y], gtid.y < 4
        else if (r >= VT_R + 4 && bot_edge) vy = fminf(((float)(j - 4) + 0.5f) * ty + 4.0f * ty, 1.0f);   // Cache[gtid.y + 8], gtid.y >= 252
        else vy = ((float)j + 0.5f) * ty;
        smp[r][threadIdx.x] = to4(sample_2d_h4(in, iw, ih, iw, uvx, vy));
    }
}
// the nine taps of output row r of the tile, down this thread's column
__device__ __forceinline__ F4 vtile_gauss9(const float4 (*smp)[VT_W], int r) {
    F4 v = f4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int i = 0; i < 9; i++) v = fma4(from4(smp[r + i][threadIdx.x]), c_gauss[i], v);
    return v;
}

__global__ __launch_bounds__(256) void k_blur_v(const pbr_half* __restrict__ in, int iw, int ih,
                                                 pbr_half* __restrict__ out, int ow, int oh, float tx, float ty) {
    __shared__ float4 smp[VT_R + 8][VT_W];
    const int x = blockIdx.x * VT_W + threadIdx.x;
    const int y0 = blockIdx.y * VT_R;
    vtile_sample(smp, in, iw, ih, x, y0, tx, ty);
    __syncthreads();
    if (x >= ow) return;
    for (int r = threadIdx.y; r < VT_R; r += 4) {
        const int y = y0 + r;
        if (y >= oh) break;
        store_h4(out + 4 * ((size_t)y * ow + x), vtile_gauss9(smp, r));
    }
}

// ---------------------------------------------------------------- final three dispatches fused: shared pieces, k_blur_v_merge
// A0 = V(B0) (blur_vertical.hlsl), S += A0 (bloom_merge.hlsl) and — optionally — the luminance histogram of the merged pixel
// (hdr_luminance_histogram.hlsl:23-59) in one pass over the frame: A0 is never written to HBM and the histogram does not re-read
// the HDR buffer.  Every intermediate is rounded exactly where the separate dispatches round, so the HDR result is bit-identical
// to the unfused chain.
__device__ __forceinline__ uint32_t luminance_bin_exact(float r, float g, float b, float min_log, float inv_range) {
    const float lum = (r * 0.2126f + g * 0.7152f) + b * 0.0722f;
    if (lum < EPSILON_F) return 0u;
    // lum >= 1e-6 is a normal number: log2f's subnormal pre-scaling never applies, so the bare v_log_f32 it wraps gives the same bits
    const float l = saturatef((__builtin_amdgcn_logf(lum) - min_log) * inv_range);
    return (uint32_t)floorf(l * 254.0f + 1.0f);
}

// Per-wave LDS histograms of a block of NT threads (thread t): cleared at the start, summed into the global one at the end.  The
// caller puts a barrier between the clear, its atomicAdds and the flush.
template <int NT, int NH, int NB>
__device__ __forceinline__ void hist_clear(uint32_t (&sh)[NH][NB], int t) {
    for (int i = t; i < NH * NB; i += NT) (&sh[0][0])[i] = 0u;
}
template <int NT, int NH, int NB>
__device__ __forceinline__ void hist_flush(const uint32_t (&sh)[NH][NB], int t, uint32_t* __restrict__ hist) {
    static_assert(NT >= NB, "one bin per thread");
    if (NT == NB || t < NB) {
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < NH; k++) sum += sh[k][t];
        if (sum) atomicAdd(&hist[t], sum);
    }
}

// The merge rounding: the V pass's fp32 result `a` rounded to fp16 as the separate pass would have stored it (A0), then the fp16 sum
// with the HDR texel.  Two variants of the same roundings, because the form decides the instructions: k_blur_hv and k_blur_v_merge
// convert component by component (the texel is read and the result written through references: returned by value, the H4 costs
// k_blur_hv 16 pack instructions); k_blur_up_poly, bound by VALU issue, rounds PAIRS in one v_cvt_pk_f16_f32 and takes the
// constant alpha's A0 (a0w, already rounded) once per thread.
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float float2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void merge_rounded(F4 a, const H4& hdr, H4& o) {
    H4 a0;
    a0.x = to_half_rn(a.x); a0.y = to_half_rn(a.y); a0.z = to_half_rn(a.z); a0.w = to_half_rn(a.w);
    const F4 s = h4f(hdr);
    o.x = to_half_rn(s.x + (float)a0.x); o.y = to_half_rn(s.y + (float)a0.y); o.z = to_half_rn(s.z + (float)a0.z); o.w = to_half_rn(s.w + (float)a0.w);
}
// two to_half_rn in one v_cvt_pk_f16_f32 (same rounding); the halves are read back out of the packed register
__device__ __forceinline__ half2v round_h2(float a, float b) {
    asm volatile("" : "+v"(a), "+v"(b));
    float2v f; f.x = a; f.y = b;
    return __builtin_convertvector(f, half2v);
}
struct alignas(8) H4Packed { half2v lo, hi; };
__device__ __forceinline__ H4Packed merge_rounded_packed(V3 a, float a0w, F4 s) {
    const half2v a01 = round_h2(a.x, a.y);
    const h16 a2 = to_half_rn(a.z);
    H4Packed o;
    o.lo = round_h2(s.x + (float)a01.x, s.y + (float)a01.y);
    o.hi = round_h2(s.z + (float)a2, s.w + a0w);
    return o;
}

template <bool HIST>
__global__ __launch_bounds__(256) void k_blur_v_merge(const pbr_half* __restrict__ in, int w, int h, float tx, float ty,
                                                       pbr_half* __restrict__ hdr, int pitch, int tiles_x, int tiles_y,
                                                       int hx0, int hy0, int hx1, int hy1, float min_log, float inv_range,
                                                       uint32_t* __restrict__ hist) {
    __shared__ float4 smp[VT_R + 8][VT_W];
    __shared__ uint32_t sh_hist[HIST ? 4 : 1][HIST ? PBR_HISTOGRAM_BINS : 1];   // persistent blocks: flushed once per block
    const int tid = threadIdx.y * VT_W + threadIdx.x;
    if (HIST) hist_clear<256>(sh_hist, tid);
    const int n_tiles = tiles_x * tiles_y;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int x = (tile % tiles_x) * VT_W + threadIdx.x;
        const int y0 = (tile / tiles_x) * VT_R;
        __syncthreads();   // previous tile's reads of smp are done (and the histogram clear on the first trip)
        vtile_sample(smp, in, w, h, x, y0, tx, ty);
        __syncthreads();
        if (x < w) {
            for (int r = threadIdx.y; r < VT_R; r += 4) {
                const int y = y0 + r;
                if (y >= h) break;
                const F4 v = vtile_gauss9(smp, r);
                pbr_half* px = hdr + 4 * ((size_t)y * pitch + x);
                H4 o;
                merge_rounded(v, *reinterpret_cast<const H4*>(px), o);
                *reinterpret_cast<H4*>(px) = o;
                if (HIST) {
                    if (x >= hx0 && x < hx1 && y >= hy0 && y < hy1)
                        atomicAdd(&sh_hist[threadIdx.y][luminance_bin_exact((float)o.x, (float)o.y, (float)o.z, min_log, inv_range)], 1u);
                }
            }
        }
    }
    if (HIST) {
        __syncthreads();
        hist_flush<256>(sh_hist, tid, hist);
    }
}

// ---------------------------------------------------------------- bloom_merge.hlsl:7-11
__global__ __launch_bounds__(256) void k_bloom_merge(pbr_half* __restrict__ hdr, int pitch, const pbr_half* __restrict__ in, int w, int h) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= w || y >= h) return;
    pbr_half* p = hdr + 4 * ((size_t)y * pitch + x);
    store_h4(p, load_h4(p) + load_h4(in + 4 * ((size_t)y * w + x)));
}

// =====================================================================================================
// Fused kernels for exact 2x pyramids (every level exactly half the one above, sizes <= 8192).
//
// With the fixed-point sampler (pbr_device.hpp::bilinear_coord) every sample position of the bloom chain then snaps to an exact
// dyadic coordinate: a same-size sample IS the texel, a 2x-down sample is the mean of a 2x2 quad, a 2x-up sample has weights
// 1/4 | 3/4 — whatever float formula produced the coordinate (the shader's group-edge formulas, `u + offset * texel`, ...).  So a
// sample is a function of its INTEGER position alone, positions outside the image read the clamped edge texel, and
//   * the prefilter's five samples per output are shared between neighbouring outputs (1.16 instead of 5 evaluations per output),
//   * the V pass's same-size sample is an exact texel of its own column, so H pass + V pass of a level fuse into one kernel whose
//     H result (rounded to fp16 exactly where the H pass would have stored it) stays in LDS; the last level adds merge + histogram.
// Results are bit-identical to the staged kernels above (tests/test_gpu_parity.py), which remain the generic path.

constexpr int PF_TW = 64, PF_TH = 16;
// Multi-view frames (pbr_bloom_histogram_views): the fused kernels take a view table and run view blockIdx.y of it in place of their own
// pointers (NoViews, an empty argument in a padding hole of the argument block: the single-view kernel, its arguments where they were).  Sizes and rectangles are the views' common ones.
struct PrefilterViews { const pbr_half* hdr[PBR_MAX_VIEWS]; pbr_half* out[PBR_MAX_VIEWS]; int pitch[PBR_MAX_VIEWS]; };
struct LevelViews {
    const pbr_half* in[PBR_MAX_VIEWS];
    const pbr_half* in2[PBR_MAX_VIEWS];
    pbr_half* out[PBR_MAX_VIEWS];
    uint32_t* hist[PBR_MAX_VIEWS];
    int out_pitch[PBR_MAX_VIEWS];
};
template <class VS = NoViews>
__global__ __launch_bounds__(256) void k_bloom_prefilter_2x(const pbr_half* __restrict__ hdr_, int w, int h, int pitch_, VS vs,
                                                              pbr_half* __restrict__ out_, OutRects rs, float threshold, float knee) {
    // (the view selection stays in the kernel body, unlike level_args below: behind a helper of either shape this instantiation's
    //  two-quad loop comes out with 40 register copies more)
    const pbr_half* __restrict__ hdr = hdr_;
    pbr_half* __restrict__ out = out_;
    int pitch = pitch_;
    if constexpr (!std::is_same_v<VS, NoViews>) { hdr = vs.hdr[blockIdx.y]; out = vs.out[blockIdx.y]; pitch = vs.pitch[blockIdx.y]; }
    __shared__ float4 pos[PF_TH + 2][PF_TW + 2];   // (colour * weight, weight) of every sample position the tile touches
    const int tid = threadIdx.x;
    int r = 0;
    while (r + 1 < rs.n && (int)blockIdx.x >= rs.first[r + 1]) r++;
    const int lb = (int)blockIdx.x - rs.first[r];
    const OutRect rc{rs.x0[r], rs.y0[r], rs.x1[r], rs.y1[r], rs.ox, rs.oy, rs.pitch};
    const int bx0 = rc.x0 + (lb % rs.tiles_x[r]) * PF_TW, by0 = rc.y0 + (lb / rs.tiles_x[r]) * PF_TH;   // tiles are laid over the output rect
    const int px0 = bx0 - 1, py0 = by0 - 1;
    // one position = the quad (2p-1, 2p) x (2q-1, 2q), weights 1/2 (position p samples u = p / ow: texel coordinate 2p - 1/2).  The four
    // texels of the NEXT position of this thread are loaded before the current one is evaluated: eight loads in flight per thread
    struct Quad { H4 a, b, c, d; };
    auto load_quad = [&](int e) {
        const int r = e / (PF_TW + 2), c = e - r * (PF_TW + 2);
        const int p = px0 + c, q = py0 + r;
        const int x0 = clampi(2 * p - 1, 0, w - 1), x1 = clampi(2 * p, 0, w - 1);
        const int y0 = clampi(2 * q - 1, 0, h - 1), y1 = clampi(2 * q, 0, h - 1);
        const H4* r0 = reinterpret_cast<const H4*>(hdr) + (size_t)y0 * pitch;
        const H4* r1 = reinterpret_cast<const H4*>(hdr) + (size_t)y1 * pitch;
        return Quad{r0[x0], r0[x1], r1[x0], r1[x1]};
    };
    constexpr int NPOS = (PF_TH + 2) * (PF_TW + 2);
    auto evaluate = [&](int e, const Quad& t) {
        const int r = e / (PF_TW + 2), c = e - r * (PF_TW + 2);
        pos[r][c] = soft_knee_sample(bilerp(h4f(t.a), h4f(t.b), h4f(t.c), h4f(t.d), 0.5f, 0.5f), threshold, knee);
    };
    // two register sets in turn (a copy `cur = nxt` would wait for the next quad's data at the end of every trip)
    Quad qa = load_quad(tid);   // tid < 256 < NPOS
    for (int e = tid; e < NPOS; e += 512) {
        const Quad qb = load_quad(min(e + 256, NPOS - 1));
        evaluate(e, qa);
        if (e + 256 < NPOS) {
            qa = load_quad(min(e + 512, NPOS - 1));
            evaluate(e + 256, qb);
        }
    }
    __syncthreads();
    const int lx = tid & 63, x = bx0 + lx;
    if (x >= rc.x1) return;
#pragma unroll
    for (int k = 0; k < PF_TH / 4; k++) {
        const int ly = (tid >> 6) + 4 * k, y = by0 + ly;
        if (y >= rc.y1) break;
        // the shader's order: centre, (-1,-1), (-1,+1), (+1,-1), (+1,+1)
        const float4 e0 = pos[ly + 1][lx + 1], e1 = pos[ly][lx], e2 = pos[ly + 2][lx], e3 = pos[ly][lx + 2], e4 = pos[ly + 2][lx + 2];
        float tr = (((e0.x + e1.x) + e2.x) + e3.x) + e4.x;
        float tg = (((e0.y + e1.y) + e2.y) + e3.y) + e4.y;
        float tb = (((e0.z + e1.z) + e2.z) + e3.z) + e4.z;
        const float tw = (((e0.w + e1.w) + e2.w) + e3.w) + e4.w;
        if (tw > 0.0f) { tr /= tw; tg /= tw; tb /= tw; }
        store_h4(out + 4 * ((size_t)(y + rc.oy) * rc.pitch + (x + rc.ox)), f4(tr, tg, tb, 1.0f));
    }
}

enum { M_SAME = 0, M_DOWN = 1, M_UP = 2 };
// source taps of integer output position p along one axis: clamped indices and the weight of the second tap
template <int MODE>
__device__ __forceinline__ void tap1d(int p, int in_size, int& i0, int& i1, float& f) {
    int a;
    if (MODE == M_SAME) { a = p; f = 0.0f; }                       // the texel itself
    else if (MODE == M_DOWN) { a = 2 * p; f = 0.5f; }             // (2p, 2p+1)
    else { a = (p >> 1) - 1 + (p & 1); f = (p & 1) ? 0.25f : 0.75f; }   // p = 2k: (k-1, k) 3/4; p = 2k+1: (k, k+1) 1/4
    i0 = clampi(a, 0, in_size - 1);
    i1 = clampi(a + 1, 0, in_size - 1);
}
struct Tap2 { H4 c00, c10, c01, c11; };
template <int MODE>
__device__ __forceinline__ Tap2 load_tap2(const pbr_half* __restrict__ in, int iw, int x0, int x1, int y0, int y1) {
    const H4* r0 = reinterpret_cast<const H4*>(in) + (size_t)y0 * iw;
    Tap2 t;
    t.c00 = r0[x0];
    if (MODE != M_SAME) {
        const H4* r1 = reinterpret_cast<const H4*>(in) + (size_t)y1 * iw;
        t.c10 = r0[x1]; t.c01 = r1[x0]; t.c11 = r1[x1];
    }
    return t;
}

// rgb-only variants: inside pbr_bloom the alpha of every chain level is one constant per level (the prefilter writes
// 1, and every later pass filters a constant field with clamp addressing), so the fused kernels filter three
// channels per pixel and push the constant through the same fp32 operations once per thread.
__device__ __forceinline__ V3 h3f(H4 h) { return v3((float)h.x, (float)h.y, (float)h.z); }
__device__ __forceinline__ V3 fma3(V3 a, float s, V3 b) { return v3(__builtin_fmaf(a.x, s, b.x), __builtin_fmaf(a.y, s, b.y), __builtin_fmaf(a.z, s, b.z)); }
template <int MODE>
__device__ __forceinline__ float4 finish_tap2_rgb(const Tap2& t, float fx, float fy) {
    if (MODE == M_SAME) return make_float4((float)t.c00.x, (float)t.c00.y, (float)t.c00.z, 0.0f);
    // weights are 1/4, 1/2 or 3/4 here — never 0, so lerp4's zero-weight select is dead: same values, fewer instructions
    const float wx0 = 1.0f - fx, wy0 = 1.0f - fy;
    const V3 top = fma3(h3f(t.c10), fx, h3f(t.c00) * wx0);
    const V3 bot = fma3(h3f(t.c11), fx, h3f(t.c01) * wx0);
    const V3 r = fma3(bot, fy, top * wy0);
    return make_float4(r.x, r.y, r.z, 0.0f);
}
__device__ __forceinline__ V3 gauss9_rgb(const float4* c) {
    V3 v = v3(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int i = 0; i < 9; i++) { const float4 e = c[i]; v = fma3(v3(e.x, e.y, e.z), c_gauss[i], v); }
    return v;
}
__device__ __forceinline__ float gauss9_const(float c) {   // the nine fused mads of gauss9 on a constant field
    float v = 0.0f;
#pragma unroll
    for (int i = 0; i < 9; i++) v = __builtin_fmaf(c, c_gauss[i], v);
    return v;
}

// H pass (+ optional second, same-size input: bloom_upsample_add) + V pass [+ merge + histogram] of one level.
// One block = one 64 x TH tile of outputs:
//   1+2. every wave owns (TH+8)/NW of the TH+8 rows the V pass will tap (rows outside the image repeat the edge).
//        It samples its rows' 72 positions (64 columns + the 4+4 halo; all global loads issued up front), then row
//        by row writes the samples to a wave-private LDS line (the H pass's Cache[]), H-gausses it and rounds to
//        fp16 exactly where the H pass stores — no block barrier: LDS operations of one wave execute in order;
//   3.   after the only barrier, V-gauss down each column from the shared fp16 tile, then store / merge into the
//        HDR buffer / histogram.
// TAIL instances: which part of the ow x oh level is merged, and where the HDR buffer sits inside it.
//   tiles  : the 64 x TH tiles (tx0 + i, ty0 + j), i < tiles_x, are walked (the whole level: tx0 = ty0 = 0);
//   merge  : only HDR texels inside [mx0,mx1) x [my0,my1) are read and updated;
//   buffer : level texel (x, y) lives at hdr[(y - by) * pitch + (x - bx)] (a whole-level buffer: bx = by = 0);
//   hist   : texels inside [hx0,hx1) x [hy0,hy1) are counted (TAIL 2).
// A single-GPU frame merges everything; a multi-GPU tile in halo mode merges (and counts) only its interior, which
// is all its HDR buffer covers beyond a 4-pixel rim.
struct TailRect { int tx0, ty0, mx0, my0, mx1, my1, bx, by, hx0, hy0, hx1, hy1; };
__device__ __forceinline__ bool merge_has_x(const TailRect& tr, int x) { return x >= tr.mx0 && x < tr.mx1; }   // the merge rect lies inside the level: implies x < ow
__device__ __forceinline__ bool merge_has(const TailRect& tr, bool has_x, int y) { return has_x && y >= tr.my0 && y < tr.my1; }
__device__ __forceinline__ bool hist_has(const TailRect& tr, int x, int y) { return x >= tr.hx0 && x < tr.hx1 && y >= tr.hy0 && y < tr.hy1; }

// what a fused level kernel works on: its own arguments (NoViews), or view blockIdx.y of the view table
struct LevelArgs { const pbr_half* in; const pbr_half* in2; pbr_half* out; uint32_t* hist; int out_pitch; };
template <class VS>
__device__ __forceinline__ LevelArgs level_args(const VS& vs, const pbr_half* in, const pbr_half* in2, pbr_half* out, uint32_t* hist, int out_pitch) {
    if constexpr (std::is_same_v<VS, NoViews>) return LevelArgs{in, in2, out, hist, out_pitch};
    else { const int v = blockIdx.y; return LevelArgs{vs.in[v], vs.in2[v], vs.out[v], vs.hist[v], vs.out_pitch[v]}; }
}

// The level's constant alpha: through the H pass (+ the second input's) and its fp16 store (t), then through the V pass (v).
// It is read at a texel that the launch's rectangle decides.  With a rectangle (tiled bloom) the producer of `in` was itself run on
// a rectangle and left texel 0 of the level untouched, so the read is at the merge rect's corner — halved for M_UP, where `in` is
// the coarser level; without a rectangle that corner is texel 0.  M_SAME / M_DOWN levels are never run on a rectangle: texel 0.
struct LevelAlpha { h16 t; float v; };
template <int MODE, bool DUAL>
__device__ __forceinline__ LevelAlpha level_alpha(const pbr_half* __restrict__ in, int iw, int ih, const pbr_half* __restrict__ in2, int ow, int oh, const TailRect& tr) {
    const size_t a_at = MODE == M_UP ? (size_t)min(tr.my0 >> 1, ih - 1) * iw + min(tr.mx0 >> 1, iw - 1) : (size_t)0;
    float alpha_h = gauss9_const((float)reinterpret_cast<const H4*>(in)[a_at].w);
    if (DUAL) alpha_h = alpha_h + gauss9_const((float)reinterpret_cast<const H4*>(in2)[(size_t)min(tr.my0, oh - 1) * ow + min(tr.mx0, ow - 1)].w);
    const h16 alpha_t = to_half_rn(alpha_h);
    return LevelAlpha{alpha_t, gauss9_const((float)alpha_t)};
}

// Lanes of one wave exchange data through LDS without a block barrier: DS operations of a wave execute in order, but the compiler
// must be told that other lanes' slots are read (per-thread alias analysis would let it hoist the loads above the store).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int MODE, bool DUAL, int TAIL, int TH, int NT, class VS = NoViews>   // TAIL 0: store; 1: merge into hdr; 2: merge + histogram
__global__ __launch_bounds__(NT, 4) void k_blur_hv(const pbr_half* __restrict__ in_, int iw, int ih,
                                                 const pbr_half* __restrict__ in2_,   // DUAL: ow x oh, same-size
                                                 pbr_half* __restrict__ out_, int ow, int oh, int out_pitch_,
                                                 int tiles_x, int n_tiles,
                                                 TailRect tr, float min_log, float inv_range, VS vs,
                                                 uint32_t* __restrict__ hist_) {
    const auto [in, in2, out, hist, out_pitch] = level_args(vs, in_, in2_, out_, hist_, out_pitch_);
    constexpr int TW = 64, SW = TW + 8, SR = TH + 8;
    constexpr int NW = NT / 64;
    constexpr int PER_T = SR / NW;                      // sampled / H-gaussed rows per wave: rows wv*PER_T .. +PER_T-1
    constexpr int PER_O = TH / NW;                      // final outputs per thread (rows wv, wv + NW, ...)
    static_assert(SR % NW == 0 && TH % NW == 0 && PER_T * 8 <= 64, "rows must split evenly over the waves; one halo tap per lane");
    __shared__ float4 sLine[DUAL ? 2 : 1][NW][SW];
    __shared__ H4 sT[SR][TW];
    __shared__ uint32_t sh_hist[TAIL == 2 ? NW : 1][TAIL == 2 ? PBR_HISTOGRAM_BINS : 1];
    const int t = threadIdx.x, lane = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);   // wave-uniform: row arithmetic stays on the scalar unit
    if (TAIL == 2) hist_clear<NT>(sh_hist, t);
    const LevelAlpha alpha = level_alpha<MODE, DUAL>(in, iw, ih, in2, ow, oh, tr);
    // 1-D grid over tiles; the histogram instance is launched with fewer blocks than tiles (each walks several) so
    // that the per-block flush of 256 global atomics stays rare
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int x0 = (tr.tx0 + tile % tiles_x) * TW, y0 = (tr.ty0 + tile / tiles_x) * TH;   // (TAIL 0 without a rectangle: tx0 = ty0 = 0)
    const int x = x0 + lane;
    // the HDR texels the merge will need: in flight from the start
    H4 hdr_in[PER_O];
    const bool in_mx = TAIL != 0 && merge_has_x(tr, x);
    if (TAIL != 0) {
#pragma unroll
        for (int k = 0; k < PER_O; k++) {
            const int y = y0 + wv + NW * k;
            if (merge_has(tr, in_mx, y)) hdr_in[k] = *reinterpret_cast<const H4*>(out + 4 * ((size_t)(y - tr.by) * out_pitch + (x - tr.bx)));
        }
    }
    // positions: columns x0-4+c (c = 0..71), rows clamp(y0-4+r) (r = 0..SR-1).  Main tap of row k: c = lane; the halo
    // columns c = 64..71 of the wave's PER_T rows are ONE extra tap: lane -> (row lane / 8, column 64 + lane % 8).
    const int r0 = wv * PER_T;
    const bool has_halo = lane < PER_T * 8;
    const int hk = lane >> 3, hc = 64 + (lane & 7);
    float4* line = sLine[0][wv];
    float4* line2 = sLine[DUAL ? 1 : 0][wv];
    {
        Tap2 htap;
        H4 up[DUAL ? PER_T : 1], hup;   // DUAL: the same-size input of bloom_upsample_add, exact texels
        float fx, hfx, hfy = 0.0f;
        float4 smp[PER_T];              // the wave's PER_T rows of samples at this lane's column (rgb)
        int ax0, ax1, bx0, bx1;
        tap1d<MODE>(x0 - 4 + lane, iw, ax0, ax1, fx);
        tap1d<MODE>(x0 - 4 + hc, iw, bx0, bx1, hfx);
        const int sx = clampi(x0 - 4 + lane, 0, ow - 1), shx = clampi(x0 - 4 + hc, 0, ow - 1);
        const int first = y0 - 4 + r0;   // wave-uniform
        // 2x-up sampling, rows that need no vertical clamping (every wave but those on the image's first / last rows): the
        // PER_T consecutive output rows blend only 4 (5) distinct input rows — output row 2m takes (m-1, m) with weight 3/4,
        // row 2m+1 takes (m, m+1) with 1/4 — and the bilinear sample lerps in x first: hrow[j] = the x-lerp of input row j
        // is computed ONCE and shared by the output rows that use it.  Same operations on the same operands as
        // finish_tap2_rgb, half the loads and converts.  (Index patterns are compile-time per parity of the first row.)
        const bool shared_rows = MODE == M_UP && first >= 1 && first + PER_T - 1 <= oh - 2;
        if (MODE == M_UP && shared_rows) {
            constexpr int NR = PER_T / 2 + 2;   // distinct input rows: 4 for PER_T = 5; 5 (even start) / 4 (odd start) for 6
            const int base = (first >> 1) - 1 + (first & 1);
            V3 hrow[NR];
            const float wx0 = 1.0f - fx;
#pragma unroll
            for (int j = 0; j < NR; j++) {
                const H4* row = reinterpret_cast<const H4*>(in) + (size_t)min(base + j, ih - 1) * iw;
                const H4 c0 = row[ax0], c1 = row[ax1];
                hrow[j] = fma3(h3f(c1), fx, h3f(c0) * wx0);
            }
            auto blend = [&](auto parity) {
                constexpr int P = decltype(parity)::value;
#pragma unroll
                for (int k = 0; k < PER_T; k++) {
                    // output row first + k = 2m (+1): input rows (i0, i0 + 1) relative to base, second-tap weight 3/4 (1/4)
                    const int odd = (P + k) & 1;
                    const int i0 = (P + k + 1) / 2 - P;          // even start: 0,1,1,2,2,3   odd start: 0,0,1,1,2,2
                    const float fyk = odd ? 0.25f : 0.75f, wy0 = 1.0f - fyk;
                    const V3 r = fma3(hrow[i0 + 1], fyk, hrow[i0] * wy0);
                    smp[k] = make_float4(r.x, r.y, r.z, 0.0f);
                }
            };
            if (first & 1) blend(std::integral_constant<int, 1>{}); else blend(std::integral_constant<int, 0>{});
#pragma unroll
            for (int k = 0; k < PER_T; k++)
                if (DUAL) up[k] = reinterpret_cast<const H4*>(in2)[(size_t)(first + k) * ow + sx];
        } else {
            Tap2 taps[PER_T];
            float fy[PER_T];
#pragma unroll
            for (int k = 0; k < PER_T; k++) {
                const int jj = clampi(first + k, 0, oh - 1);
                int ay0, ay1;
                tap1d<MODE>(jj, ih, ay0, ay1, fy[k]);
                taps[k] = load_tap2<MODE>(in, iw, ax0, ax1, ay0, ay1);
                if (DUAL) up[k] = reinterpret_cast<const H4*>(in2)[(size_t)jj * ow + sx];
            }
#pragma unroll
            for (int k = 0; k < PER_T; k++) smp[k] = finish_tap2_rgb<MODE>(taps[k], fx, fy[k]);
        }
        if (has_halo) {
            const int jj = clampi(first + hk, 0, oh - 1);
            int ay0, ay1;
            tap1d<MODE>(jj, ih, ay0, ay1, hfy);
            htap = load_tap2<MODE>(in, iw, bx0, bx1, ay0, ay1);
            if (DUAL) hup = reinterpret_cast<const H4*>(in2)[(size_t)jj * ow + shx];
        }
#pragma unroll
        for (int k = 0; k < PER_T; k++) {
            line[lane] = smp[k];
            if (DUAL) line2[lane] = make_float4((float)up[k].x, (float)up[k].y, (float)up[k].z, 0.0f);
            if (has_halo && hk == k) {
                line[hc] = finish_tap2_rgb<MODE>(htap, hfx, hfy);
                if (DUAL) line2[hc] = make_float4((float)hup.x, (float)hup.y, (float)hup.z, 0.0f);
            }
            wave_sync();
            V3 g = gauss9_rgb(line + lane);
            if (DUAL) g = g + gauss9_rgb(line2 + lane);   // bloom_upsample_add: lower first, then upper
            wave_sync();
            H4 th;   // the H pass's fp16 store
            th.x = to_half_rn(g.x); th.y = to_half_rn(g.y); th.z = to_half_rn(g.z); th.w = alpha.t;
            sT[r0 + k][lane] = th;
        }
    }
    __syncthreads();
    // ---- phase 3: V-gauss + tail
#pragma unroll
    for (int k = 0; k < PER_O; k++) {
        const int r = wv + NW * k, y = y0 + r;
        if (x >= ow || y >= oh) continue;
        V3 a3 = v3(0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int i = 0; i < 9; i++) a3 = fma3(h3f(sT[r + i][lane]), c_gauss[i], a3);
        const F4 a = f4(a3.x, a3.y, a3.z, alpha.v);
        if (TAIL == 0) {
            store_h4(out + 4 * ((size_t)y * out_pitch + x), a);
        } else {
            if (!(merge_has(tr, in_mx, y))) continue;
            H4 o;
            merge_rounded(a, hdr_in[k], o);
            *reinterpret_cast<H4*>(out + 4 * ((size_t)(y - tr.by) * out_pitch + (x - tr.bx))) = o;
            if (TAIL == 2) {
                if (hist_has(tr, x, y))
                    atomicAdd(&sh_hist[wv][luminance_bin_exact((float)o.x, (float)o.y, (float)o.z, min_log, inv_range)], 1u);
            }
        }
    }
    if (tile + (int)gridDim.x < n_tiles) __syncthreads();   // the next tile overwrites sT
    }
    if (TAIL == 2) {
        __syncthreads();
        hist_flush<NT>(sh_hist, t, hist);
    }
}

// ---------------------------------------------------------------- 2x-up levels of large images: k_blur_up_poly
// texel `byte_off / 8` of a half4 image: a (wave-uniform or not) base + an UNSIGNED 32-bit byte offset, the form that loads as
// `global_load_dwordx2 v, v_off, s[base]` — a signed index makes every load pay a 64-bit vector add (slow issue class, §4.7).
// Images here are < 4 GiB (8 192^2 half4 = 512 MB).
__device__ __forceinline__ H4 ld_h4(const void* base, uint32_t byte_off) {
    return *reinterpret_cast<const H4*>(reinterpret_cast<const char*>(base) + byte_off);
}
// the nine taps of the two outputs of a lane from the five pair entries e[0..4] of one channel
__device__ __forceinline__ void gauss9_pair(const float2* e, float& ge, float& go) {
    const float s[10] = {e[0].x, e[0].y, e[1].x, e[1].y, e[2].x, e[2].y, e[3].x, e[3].y, e[4].x, e[4].y};
    float a = 0.0f, b = 0.0f;
#pragma unroll
    for (int i = 0; i < 9; i++) { a = __builtin_fmaf(s[i], c_gauss[i], a); b = __builtin_fmaf(s[i + 1], c_gauss[i], b); }
    ge = a; go = b;
}

// k_blur_up_poly: the passes of k_blur_hv<M_UP, ...> on 128 x TH tiles, one block (512 threads, 8 waves) per tile, rearranged so
// that the 2x upsample costs little.  The shader evaluates every one of the nine taps of a fine-grid output as a bilinear 2x-up
// sample of the coarse level (weights 1/4 | 3/4 in x and in y), 9 taps x (TH + 8) fine rows.  The upsample and the blur are both
// linear and the upsample's weights are periodic, so the H blur of the upsampled row is two FIXED six-tap filters on the COARSE
// row — even outputs 2p tap c[p-3 .. p+2], odd outputs 2p+1 tap c[p-2 .. p+3] (coefficients below) — and the y half of the
// bilinear sample commutes with the H blur: filter the ~TH/2 + 6 coarse rows once, THEN blend neighbouring filtered rows with
// 1/4 | 3/4 into the fine rows.  Per fine output and channel that is ~6 x 22/40 + 2 multiply-adds for the H pass instead of
// 9 + the four of the bilinear sample; a lane loads ONE coarse texel per coarse row and reads seven 8-byte LDS entries per coarse row.
//   * DUAL: a lane owns the fine column PAIR (2p, 2p+1) of the same-size input's row, held in LDS as float2 pairs; its two outputs
//     tap the five entries lane .. lane+4 (gauss9_pair).
//   * V pass: a thread owns a column and TH/4 CONSECUTIVE rows, so the rows it taps overlap: TH/4 + 8 reads of the fp16 tile
//     for TH/4 outputs instead of nine per output.
// Not the shader's operation order, hence not bit-identical to the oracle: the fp32 value in front of the H pass's fp16 store
// differs by a few fp32 ulps, i.e. the stored fp16 texel differs by one fp16 ULP on ~5e-5 of the texels (SURVEY 8c allows <= 1
// fp16 ULP per bloom stage; tests/test_gpu_parity.py holds every stage to that and the whole chain to <= 2).  The sum is rounded to
// fp16 exactly where bloom_upsample_add / blur_horizontal store it; the V pass and the tail take k_blur_hv's operation order.
// Clamp addressing: a tap outside the coarse level reads the edge texel — the same linear map as the shader's clamp of the
// sample position (every fine position outside the level samples the pure edge texel either way).
namespace poly {
constexpr double G[9] = {0.0148, 0.0459, 0.1050, 0.1941, 0.2803, 0.1941, 0.1050, 0.0459, 0.0148};   // blur.hlsli:17
constexpr double g(int k) { return (k < -4 || k > 4) ? 0.0 : G[k + 4]; }
// coefficient of c[p + j] in the EVEN output 2p: sum_k g(k) * [weight of c[p + j] in the 2x-up sample at fine position 2p + k];
// the odd output 2p + 1 takes c[p + j] with E(-j)   (j = -3 .. 2 resp. -2 .. 3; both sets sum to 0.9999 like the nine weights)
constexpr float E(int j) { return (float)(0.75 * g(2 * j) + 0.25 * g(2 * j + 2) + 0.75 * g(2 * j + 1) + 0.25 * g(2 * j - 1)); }
}  // namespace poly

template <bool DUAL, int TAIL, int TH, class VS = NoViews>
__global__ __launch_bounds__(512, 4) void k_blur_up_poly(const pbr_half* __restrict__ in_, int iw, int ih,
                                                          const pbr_half* __restrict__ in2_,   // DUAL: ow x oh, same-size
                                                          pbr_half* __restrict__ out_, int ow, int oh, int out_pitch_,
                                                          int tiles_x, int n_tiles,
                                                          TailRect tr, float min_log, float inv_range, VS vs,
                                                          uint32_t* __restrict__ hist_) {
    const auto [in, in2, out, hist, out_pitch] = level_args(vs, in_, in2_, out_, hist_, out_pitch_);
    constexpr int TW = 128, NP = TW / 2 + 4, NC = TW / 2 + 6, SR = TH + 8, NT = 512, NW = NT / 64;
    constexpr int NPAIR = TH / 2 + 5;                 // coarse row pairs (m, m + 1) whose two blends (fine rows 2m + 1, 2m + 2) the tile's SR rows need
    constexpr int PPW = (NPAIR + NW - 1) / NW;        // pairs per wave; wave w: pairs w * PPW .. (the last waves may hold fewer, or none)
    constexpr int PER_O = TH / 4;                     // V outputs per thread: column t & 127, rows (t >> 7) * PER_O ..
    static_assert(TH % 4 == 0 && (PPW + 1) * 6 <= 64 && 2 * PPW * 4 <= 64, "one halo entry per lane");
    __shared__ H4 sLineC[NW][NC + 2];                 // one coarse row per wave at a time: entry e = coarse column x0 / 2 - 3 + e
    __shared__ float2 sLineU[DUAL ? NW : 1][3][NP];   // DUAL: the same-size input's fine row as column pairs (gauss9_pair)
    __shared__ H4 sT[SR][TW];
    __shared__ uint32_t sh_hist[TAIL == 2 ? NW : 1][TAIL == 2 ? PBR_HISTOGRAM_BINS : 1];
    // two blocks (2 x 8 waves = the 4 waves per SIMD of the launch bounds) must fit a CU's 160 KiB of LDS: an instantiation that does not
    // would still build — gfx950 allows one block the whole 160 KiB — and silently run at half the occupancy
    static_assert(sizeof(sLineC) + sizeof(sLineU) + sizeof(sT) + sizeof(sh_hist) <= 80 * 1024, "k_blur_up_poly: two blocks per CU no longer fit the LDS");
    const int t = threadIdx.x, lane = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int vc = t & 127, vg = __builtin_amdgcn_readfirstlane(t >> 7);
    if (TAIL == 2) hist_clear<NT>(sh_hist, t);
    const LevelAlpha alpha = level_alpha<M_UP, DUAL>(in, iw, ih, in2, ow, oh, tr);
    const float a0w = (float)to_half_rn(alpha.v);
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int x0 = (tr.tx0 + tile % tiles_x) * TW, y0 = (tr.ty0 + tile / tiles_x) * TH;   // (TAIL 0 without a rectangle: tx0 = ty0 = 0)
    const int xv = x0 + vc, rbase = vg * PER_O;
    H4 hdr_in[PER_O];
    const bool in_mx = TAIL != 0 && merge_has_x(tr, xv);
    char* const hdr_row0 = reinterpret_cast<char*>(out) + (ptrdiff_t)(y0 + rbase - tr.by) * out_pitch * 8;
    const uint32_t hdr_x = (uint32_t)(xv - tr.bx) * 8u;
    const size_t hdr_pitch = (size_t)out_pitch * 8u;
    // ---- H pass.  Wave w owns the coarse row pairs i = w * PPW .. + PPW - 1 (i < NPAIR): coarse rows cb + i and cb + i + 1, cb = y0 / 2 - 3;
    // pair i blends into the tile's fp16 rows 2i - 1 (fine row y0 - 5 + 2i, odd) and 2i (even); rows -1 and SR do not exist.
    {
        const int i_first = wv * PPW;
        const int n_pairs = min(PPW, NPAIR - i_first);                        // wave-uniform; <= 0: nothing to do for this wave
        const int cb = (y0 >> 1) - 3 + i_first;                               // first coarse row of the wave
        const uint32_t ccol = (uint32_t)clampi((x0 >> 1) - 3 + lane, 0, iw - 1) * 8u;
        H4 cr[PPW + 1], chalo{};                                              // the wave's coarse rows at this lane's column; one halo entry
        const int hk = lane / 6, hq = 64 + lane % 6;                          // halo: lane -> (row lane / 6, entry 64 + lane % 6), lanes 0 .. 6 (PPW + 1) - 1
        const bool has_halo = lane < 6 * (PPW + 1);
        H4 upE[DUAL ? 2 * PPW : 1], upO[DUAL ? 2 * PPW : 1], hupE{}, hupO{};
        const int uk = lane >> 2, uq = 64 + (lane & 3);                       // DUAL halo: lane -> (fine row lane / 4 of the wave's 2 PPW, pair entry 64 + lane % 4)
        const bool has_uhalo = DUAL && lane < 8 * PPW;
        if (n_pairs > 0) {
#pragma unroll
            for (int k = 0; k <= PPW; k++) {
                const char* row = reinterpret_cast<const char*>(in) + (size_t)clampi(cb + k, 0, ih - 1) * iw * 8u;   // wave-uniform: a scalar base
                cr[k] = ld_h4(row, ccol);
            }
            if (has_halo) {
                const char* row = reinterpret_cast<const char*>(in) + (size_t)clampi(cb + hk, 0, ih - 1) * iw * 8u;
                chalo = ld_h4(row, (uint32_t)clampi((x0 >> 1) - 3 + hq, 0, iw - 1) * 8u);
            }
            if (DUAL) {
                const int sxe = clampi(x0 - 4 + 2 * lane, 0, ow - 1), sxo = clampi(x0 - 3 + 2 * lane, 0, ow - 1);
#pragma unroll
                for (int k = 0; k < 2 * PPW; k++) {   // fine rows of the wave: tile row 2 i_first - 1 + k
                    const char* row = reinterpret_cast<const char*>(in2) + (size_t)clampi(y0 - 4 + 2 * i_first - 1 + k, 0, oh - 1) * ow * 8u;
                    upE[k] = ld_h4(row, (uint32_t)sxe * 8u); upO[k] = ld_h4(row, (uint32_t)sxo * 8u);
                }
                if (has_uhalo) {
                    const uint32_t row = (uint32_t)(clampi(y0 - 4 + 2 * i_first - 1 + uk, 0, oh - 1) * ow) * 8u;
                    hupE = ld_h4(in2, row + (uint32_t)clampi(x0 - 4 + 2 * uq, 0, ow - 1) * 8u); hupO = ld_h4(in2, row + (uint32_t)clampi(x0 - 3 + 2 * uq, 0, ow - 1) * 8u);
                }
            }
        }
        // the HDR texels of the merge: issued AFTER the level's texels (loads return in order), consumed after the H pass
        if (TAIL != 0) {
#pragma unroll
            for (int k = 0; k < PER_O; k++) {
                const int y = y0 + rbase + k;
                if (merge_has(tr, in_mx, y)) hdr_in[k] = ld_h4(hdr_row0 + k * hdr_pitch, hdr_x);
            }
        }
        if (n_pairs > 0) {
            H4* line = sLineC[wv];
            float2 (*lineU)[NP] = sLineU[DUAL ? wv : 0];
            V3 pE = v3(0.0f, 0.0f, 0.0f), pO = pE;   // the previous coarse row, H-filtered: even / odd fine column of the lane
#pragma unroll
            for (int k = 0; k <= PPW; k++) {
                if (k > n_pairs) break;              // wave-uniform
                line[lane] = cr[k];
                if (has_halo && hk == k) line[hq] = chalo;
                wave_sync();
                V3 e[7];
#pragma unroll
                for (int j = 0; j < 7; j++) e[j] = h3f(line[lane + j]);
                wave_sync();
                // even output 2p: c[p-3 .. p+2] = e[0 .. 5] with E(-3 .. 2); odd output 2p + 1: c[p-2 .. p+3] = e[1 .. 6] with E(2 .. -3)
                constexpr float PE[6] = {poly::E(-3), poly::E(-2), poly::E(-1), poly::E(0), poly::E(1), poly::E(2)};
                V3 cE = v3(0.0f, 0.0f, 0.0f), cO = cE;
#pragma unroll
                for (int j = 0; j < 6; j++) { cE = fma3(e[j], PE[j], cE); cO = fma3(e[j + 1], PE[5 - j], cO); }
                if (k > 0) {
#pragma unroll
                    for (int half = 0; half < 2; half++) {
                        const int r = 2 * (i_first + k - 1) - 1 + half;      // tile row of this blend (wave-uniform)
                        if (r < 0 || r >= SR) continue;
                        // fine row 2m + 1: (m, m + 1) with second-tap weight 1/4; fine row 2m + 2: 3/4 (tap1d<M_UP>; the sampler's lerp form)
                        const float fy = half ? 0.75f : 0.25f, wy0 = 1.0f - fy;
                        V3 bE = fma3(cE, fy, pE * wy0), bO = fma3(cO, fy, pO * wy0);
                        if (DUAL) {   // bloom_upsample_add: lower first, then upper — the same-size input's nine taps on this fine row
                            const int u = 2 * (k - 1) + half;
                            lineU[0][lane] = make_float2((float)upE[u].x, (float)upO[u].x); lineU[1][lane] = make_float2((float)upE[u].y, (float)upO[u].y);
                            lineU[2][lane] = make_float2((float)upE[u].z, (float)upO[u].z);
                            if (has_uhalo && uk == u) {
                                lineU[0][uq] = make_float2((float)hupE.x, (float)hupO.x); lineU[1][uq] = make_float2((float)hupE.y, (float)hupO.y);
                                lineU[2][uq] = make_float2((float)hupE.z, (float)hupO.z);
                            }
                            wave_sync();
                            V3 uE, uO;
                            gauss9_pair(lineU[0] + lane, uE.x, uO.x); gauss9_pair(lineU[1] + lane, uE.y, uO.y); gauss9_pair(lineU[2] + lane, uE.z, uO.z);
                            wave_sync();
                            bE = bE + uE; bO = bO + uO;
                        }
                        struct alignas(16) H8 { H4 a, b; } th;   // the H pass's fp16 store, both columns of the lane
                        th.a.x = to_half_rn(bE.x); th.a.y = to_half_rn(bE.y); th.a.z = to_half_rn(bE.z); th.a.w = alpha.t;
                        th.b.x = to_half_rn(bO.x); th.b.y = to_half_rn(bO.y); th.b.z = to_half_rn(bO.z); th.b.w = alpha.t;
                        *reinterpret_cast<H8*>(&sT[r][2 * lane]) = th;
                    }
                }
                pE = cE; pO = cO;
            }
        }
    }
    __syncthreads();
    // ---- V-gauss over a sliding window of the fp16 tile + tail (k_blur_hv's operation order)
    {
        H4 win[PER_O + 8];
#pragma unroll
        for (int i = 0; i < PER_O + 8; i++) win[i] = sT[rbase + i][vc];
#pragma unroll
        for (int k = 0; k < PER_O; k++) {
            const int y = y0 + rbase + k;
            if (xv >= ow || y >= oh) continue;
            V3 a3 = v3(0.0f, 0.0f, 0.0f);
#pragma unroll
            for (int i = 0; i < 9; i++) a3 = fma3(h3f(win[k + i]), c_gauss[i], a3);
            const F4 a = f4(a3.x, a3.y, a3.z, alpha.v);
            if (TAIL == 0) {
                store_h4(out + 4 * ((size_t)y * out_pitch + xv), a);
            } else {
                if (!(merge_has(tr, in_mx, y))) continue;
                const H4Packed o = merge_rounded_packed(a3, a0w, h4f(hdr_in[k]));
                *reinterpret_cast<H4Packed*>(hdr_row0 + k * hdr_pitch + hdr_x) = o;
                if (TAIL == 2) {
                    if (hist_has(tr, xv, y))
                        atomicAdd(&sh_hist[wv][luminance_bin_exact((float)o.lo.x, (float)o.lo.y, (float)o.hi.x, min_log, inv_range)], 1u);
                }
            }
        }
    }
    if (tile + (int)gridDim.x < n_tiles) __syncthreads();   // the next tile overwrites sT
    }
    if (TAIL == 2) {
        __syncthreads();
        hist_flush<NT>(sh_hist, t, hist);
    }
}

// ---------------------------------------------------------------- the pyramid's small end inside one up-pass launch: k_bloom_small_end
// One block = one 64 x 16 tile of an up-pass (k_blur_hv<M_UP, true, 0, 16>'s), with the DEPTH smaller levels under it recomputed in LDS
// on the region the tile depends on, so that their launches go: no block waits for another.
//   DEPTH 1: the tile is level 3's; the level-4 texels it taps (what k_blur_hv<M_DOWN> of level 3 -> 4 stores) come first.
//   DEPTH 2: the tile is level 2's; level 4, then level 3's up-pass result on the region the tile taps, then the tile.
// `a_lo` is chain A of the level that is downsampled (level 3), `a_mid` chain A of level 2 (DEPTH 2), `out` chain B of the tile's level.
// The regions follow from tap1d<M_UP> (a tile origin is a multiple of 64 x 16): positions x0 - 4 .. x0 + 67 tap the 38 columns
// x0 / 2 - 3 .. of the level below, rows y0 - 4 .. y0 + 19 its 14 rows y0 / 2 - 3 ..; a 38 x 14 region at (32 n - 3, 8 m - 3) taps the
// 24 x 12 texels at (16 n - 4, 4 m - 4) of the level below it.  A region may hang over its level's edge: those texels are computed like
// the others (taps clamp as in k_blur_hv: columns by tap index, rows by position) and never read, because every tap index is clamped.
// Every stage is k_blur_hv's three steps with a block barrier between them — samples (finish_tap2_rgb; the same-size input's texels
// stay fp16: exact), H gauss + the fp16 rounding of the H pass's store, V gauss + the fp16 rounding of the level's store — in the same
// operation order on the same operands, so every value is what the separate launches compute.
namespace small_end {
constexpr int NT = 512, TW = 64, TH = 16;
constexpr int R1W = 38, R1H = 14;   // the region under a tile: 72 x 24 positions from an even origin tap n / 2 + 2 texels
constexpr int R2W = 24, R2H = 12;   // the region under that: 46 x 22 positions from an odd origin tap n / 2 + 1 texels
}  // namespace small_end
// the nine taps down a fp16 column / along a fp16 row: k_blur_hv's V pass, and its second H input
__device__ __forceinline__ V3 gauss9_h(const H4* c, int stride) {
    V3 v = v3(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int i = 0; i < 9; i++) v = fma3(h3f(c[i * stride]), c_gauss[i], v);
    return v;
}
// level_alpha on values: the input's alpha (and the second input's) through the H pass, its fp16 store and the V pass
template <bool DUAL>
__device__ __forceinline__ LevelAlpha level_alpha_of(float in_w, float in2_w) {
    float alpha_h = gauss9_const(in_w);
    if (DUAL) alpha_h = alpha_h + gauss9_const(in2_w);
    const h16 alpha_t = to_half_rn(alpha_h);
    return LevelAlpha{alpha_t, gauss9_const((float)alpha_t)};
}
// samples of a MODE level at positions (px0 + c, clamp(py0 + r)), c < SW, r < SR, of the output level (height oh): the input level
// (iw x ih) is `src`, whose texel (x, y) is src[(y - sy0) * spitch + (x - sx0)] (global: the level itself; LDS: a region of it)
template <int MODE, int SW, int SR>
__device__ __forceinline__ void se_sample(float4* sS, const H4* src, int spitch, int sx0, int sy0, int iw, int ih, int px0, int py0, int oh, int t) {
    constexpr int N = SW * SR, TRIPS = (N + small_end::NT - 1) / small_end::NT;
    Tap2 tp[TRIPS];
    float fx[TRIPS], fy[TRIPS];
#pragma unroll
    for (int k = 0; k < TRIPS; k++) {
        const int e = min(t + k * small_end::NT, N - 1);
        const int r = e / SW, c = e - r * SW;
        int ax0, ax1, ay0, ay1;
        tap1d<MODE>(px0 + c, iw, ax0, ax1, fx[k]);
        tap1d<MODE>(clampi(py0 + r, 0, oh - 1), ih, ay0, ay1, fy[k]);
        const int o0 = (ay0 - sy0) * spitch - sx0, o1 = (ay1 - sy0) * spitch - sx0;
        tp[k].c00 = src[o0 + ax0]; tp[k].c10 = src[o0 + ax1]; tp[k].c01 = src[o1 + ax0]; tp[k].c11 = src[o1 + ax1];
    }
#pragma unroll
    for (int k = 0; k < TRIPS; k++) {
        const int e = t + k * small_end::NT;
        if (e < N) sS[e] = finish_tap2_rgb<MODE>(tp[k], fx[k], fy[k]);
    }
}
// the same-size second input (ow x oh, global) at the same positions, clamped to the level both ways: exact texels
template <int SW, int SR>
__device__ __forceinline__ void se_second(H4* sU, const pbr_half* __restrict__ in2, int ow, int oh, int px0, int py0, int t) {
    constexpr int N = SW * SR, TRIPS = (N + small_end::NT - 1) / small_end::NT;
    H4 u[TRIPS];
#pragma unroll
    for (int k = 0; k < TRIPS; k++) {
        const int e = min(t + k * small_end::NT, N - 1);
        const int r = e / SW, c = e - r * SW;
        u[k] = reinterpret_cast<const H4*>(in2)[(size_t)clampi(py0 + r, 0, oh - 1) * ow + clampi(px0 + c, 0, ow - 1)];
    }
#pragma unroll
    for (int k = 0; k < TRIPS; k++) {
        const int e = t + k * small_end::NT;
        if (e < N) sU[e] = u[k];
    }
}
// H gauss of RW x SR outputs from (RW + 8) x SR samples (+ the second input's), rounded to fp16 where the H pass stores
template <bool DUAL, int RW, int SR>
__device__ __forceinline__ void se_hpass(H4* sT, const float4* sS, const H4* sU, h16 alpha_t, int t) {
    for (int e = t; e < RW * SR; e += small_end::NT) {
        const int r = e / RW, c = e - r * RW;
        V3 g = gauss9_rgb(sS + r * (RW + 8) + c);
        if (DUAL) g = g + gauss9_h(sU + r * (RW + 8) + c, 1);   // bloom_upsample_add: lower first, then upper
        H4 th;
        th.x = to_half_rn(g.x); th.y = to_half_rn(g.y); th.z = to_half_rn(g.z); th.w = alpha_t;
        sT[e] = th;
    }
}
// V gauss of RW x RH outputs from RW x (RH + 8) fp16 rows into an LDS region, rounded to fp16 where the level is stored
template <int RW, int RH>
__device__ __forceinline__ void se_vpass(H4* sL, const H4* sT, float alpha_v, int t) {
    for (int e = t; e < RW * RH; e += small_end::NT) {
        const V3 a = gauss9_h(sT + e, RW);
        H4 o;
        o.x = to_half_rn(a.x); o.y = to_half_rn(a.y); o.z = to_half_rn(a.z); o.w = to_half_rn(alpha_v);
        sL[e] = o;
    }
}

template <int DEPTH>
__global__ __launch_bounds__(small_end::NT, 4) void k_bloom_small_end(const pbr_half* __restrict__ a_lo, int lw, int lh,      // chain A level 3
                                                                    const pbr_half* __restrict__ a_mid,                     // chain A level 2 (DEPTH 2)
                                                                    pbr_half* __restrict__ out, int ow, int oh, int tiles_x) {
    using namespace small_end;
    static_assert(DEPTH == 1 || DEPTH == 2, "one or two levels under the tile");
    // the tile's samples; the region of the level below it; (DEPTH 2) the region below that.  R1 is the level the down pass makes.
    constexpr int S0W = TW + 8, S0R = TH + 8;
    constexpr int S1W = R1W + 8, S1R = R1H + 8, S2W = R2W + 8, S2R = R2H + 8;   // samples 46 x 22 and 32 x 20
    static_assert(R1W == (TW + 8) / 2 + 2 && R1H == (TH + 8) / 2 + 2 && R2W == S1W / 2 + 1 && R2H == S1R / 2 + 1, "regions of a 64 x 16 tile");
    constexpr int NS = S0W * S0R;                                       // the largest stage is the tile's own
    constexpr int NU_MID = DEPTH == 2 ? S1W * S1R : 1;
    __shared__ float4 sS[NS];                                           // samples of a stage's first input
    __shared__ H4 sU[NS];                                               // the tile stage's second input
    __shared__ H4 sUmid[NU_MID];                                        // DEPTH 2: the middle stage's second input
    __shared__ H4 sT[TW * S0R];                                         // a stage's H result
    __shared__ H4 sR1[R1W * R1H];                                       // the finished region under the tile
    __shared__ H4 sR2[DEPTH == 2 ? R2W * R2H : 1];                      // DEPTH 2: the level-4 region
    static_assert(sizeof(sS) + sizeof(sU) + sizeof(sUmid) + sizeof(sT) + sizeof(sR1) + sizeof(sR2) <= 80 * 1024, "k_bloom_small_end: two blocks per CU");
    const int t = threadIdx.x;
    const int x0 = ((int)blockIdx.x % tiles_x) * TW, y0 = ((int)blockIdx.x / tiles_x) * TH;
    const int r1x = (x0 >> 1) - 3, r1y = (y0 >> 1) - 3;                 // origin of the region under the tile
    const int w4 = lw >> 1, h4 = lh >> 1;                               // level 4
    // the constant alpha of every level on the way (level_alpha): level 4 from chain A level 3, then each up-pass from the stored
    // alpha of the level below and chain A of its own level
    const float lo_w = (float)reinterpret_cast<const H4*>(a_lo)[0].w;
    const LevelAlpha al4 = level_alpha_of<false>(lo_w, 0.0f);
    const LevelAlpha al3 = level_alpha_of<true>((float)to_half_rn(al4.v), lo_w);
    if constexpr (DEPTH == 1) {
        // ---- level 4 on R1 (the tile is level 3's: ow x oh = lw x lh), from chain A level 3 in global memory
        se_sample<M_DOWN, S1W, S1R>(sS, reinterpret_cast<const H4*>(a_lo), lw, 0, 0, lw, lh, r1x - 4, r1y - 4, h4, t);
        se_second<S0W, S0R>(sU, a_lo, ow, oh, x0 - 4, y0 - 4, t);
        __syncthreads();
        se_hpass<false, R1W, S1R>(sT, sS, nullptr, al4.t, t);
        __syncthreads();
        se_vpass<R1W, R1H>(sR1, sT, al4.v, t);
        __syncthreads();
    } else {
        const int r2x = (x0 >> 2) - 4, r2y = (y0 >> 2) - 4;             // origin of the level-4 region
        se_sample<M_DOWN, S2W, S2R>(sS, reinterpret_cast<const H4*>(a_lo), lw, 0, 0, lw, lh, r2x - 4, r2y - 4, h4, t);
        se_second<S1W, S1R>(sUmid, a_lo, lw, lh, r1x - 4, r1y - 4, t);
        se_second<S0W, S0R>(sU, a_mid, ow, oh, x0 - 4, y0 - 4, t);
        __syncthreads();
        se_hpass<false, R2W, S2R>(sT, sS, nullptr, al4.t, t);
        __syncthreads();
        se_vpass<R2W, R2H>(sR2, sT, al4.v, t);
        __syncthreads();
        // ---- level 3's up-pass on R1: level 4 from sR2, chain A level 3 from sUmid
        se_sample<M_UP, S1W, S1R>(sS, sR2, R2W, r2x, r2y, w4, h4, r1x - 4, r1y - 4, lh, t);
        __syncthreads();
        se_hpass<true, R1W, S1R>(sT, sS, sUmid, al3.t, t);
        __syncthreads();
        se_vpass<R1W, R1H>(sR1, sT, al3.v, t);
        __syncthreads();
    }
    // ---- the tile: k_blur_hv<M_UP, true, 0, 16> with the level below from sR1
    const LevelAlpha al = DEPTH == 1 ? al3 : level_alpha_of<true>((float)to_half_rn(al3.v), (float)reinterpret_cast<const H4*>(a_mid)[0].w);
    se_sample<M_UP, S0W, S0R>(sS, sR1, R1W, r1x, r1y, ow >> 1, oh >> 1, x0 - 4, y0 - 4, oh, t);
    __syncthreads();
    se_hpass<true, TW, S0R>(sT, sS, sU, al.t, t);
    __syncthreads();
    for (int e = t; e < TW * TH; e += NT) {
        const int x = x0 + (e & (TW - 1)), y = y0 + e / TW;
        if (x >= ow || y >= oh) continue;
        const V3 a = gauss9_h(sT + e, TW);
        store_h4(out + 4 * ((size_t)y * ow + x), f4(a.x, a.y, a.z, al.v));
    }
}

// ---------------------------------------------------------------- launch
// k_blur_h of in (+ in2: DUAL) into out (ow x oh).  A block pipelines as many rows as keep >= ~2048 blocks (8 per CU) in the grid
template <bool DUAL>
static pbr_status launch_blur_h(pbr_ctx* ctx, const pbr_half* in, uint32_t iw, uint32_t ih, const pbr_half* in2, uint32_t iw2, uint32_t ih2,
                                pbr_half* out, uint32_t ow, uint32_t oh) {
    const uint64_t row_blocks = (uint64_t)((ow + 255) / 256) * oh;
    int rows = (int)(row_blocks / 2048);
    rows = rows < 1 ? 1 : (rows > HB_MAX_ROWS ? HB_MAX_ROWS : rows);
    hipLaunchKernelGGL(k_blur_h<DUAL>, dim3((ow + 255) / 256, (oh + rows - 1) / rows), dim3(256), 0, ctx->stream, in, (int)iw, (int)ih, in2, (int)iw2, (int)ih2,
                       out, (int)ow, (int)oh, 1.0f / (float)ow, 1.0f / (float)oh, rows);
    return launched(ctx, DUAL ? "k_blur_h<dual>" : "k_blur_h");
}

// fast-path preconditions: the level below is exactly half, and the size keeps every snapped sample coordinate
// on its dyadic value (coordinate error ~4 * 2^-24 * size must stay below half a 1/256 step)
static bool exact_half(uint32_t n) { return (n & 1u) == 0u && n <= 8192u; }

// TailRect of a fused level of ow x oh from the launch's three optional rectangles.  rect: histogram rect {x,y,w,h} (default: none);
// merge_rect: HDR texels to merge (default: the whole level); buf_origin: level coordinates of out[0] (default 0,0).  The first
// tile (tx0, ty0) depends on the tile size: launch_hv sets it with the kernel it chooses.
static TailRect tail_rect(uint32_t ow, uint32_t oh, const uint32_t* rect, const uint32_t* merge_rect, const uint32_t* buf_origin) {
    TailRect tr{};
    if (rect) { tr.hx0 = (int)rect[0]; tr.hy0 = (int)rect[1]; tr.hx1 = (int)(rect[0] + rect[2]); tr.hy1 = (int)(rect[1] + rect[3]); }
    tr.mx1 = (int)ow; tr.my1 = (int)oh;
    if (merge_rect) {
        tr.mx0 = (int)merge_rect[0]; tr.my0 = (int)merge_rect[1];
        tr.mx1 = (int)(merge_rect[0] + merge_rect[2]); tr.my1 = (int)(merge_rect[1] + merge_rect[3]);
    }
    if (buf_origin) { tr.bx = (int)buf_origin[0]; tr.by = (int)buf_origin[1]; }
    return tr;
}
// the tw x th tiles of the level that intersect the merge rect (a launch without one: every tile of the level)
struct TileGrid { int tx0, ty0, tiles_x, n; };
static TileGrid tile_grid(const TailRect& tr, int tw, int th) {
    const int tx0 = tr.mx0 / tw, ty0 = tr.my0 / th, tiles_x = (tr.mx1 + tw - 1) / tw - tx0;
    return TileGrid{tx0, ty0, tiles_x, tiles_x * ((tr.my1 + th - 1) / th - ty0)};
}

// The kernel choice of a fused level, from the tiles of its merge rect.  2x-up levels big enough to fill the chip with 128 x 32 tiles:
// k_blur_up_poly.  Else k_blur_hv: 64 x 32 tiles when the level fills the chip that way; 64 x 16 below, where a level is latency-bound
// (one tile's dependent chain + the launch) and 3 H rows per wave, 2 outputs per thread shorten the chain.  Whether the polyphase
// kernel is taken never, by that size or always is the caller's: launch_hv and bloom_pass read PBR_BLOOM_WIDE=0|1 differently.
enum LevelKernel { K_POLY, K_HV32, K_HV16 };
enum PolyRule { POLY_NEVER, POLY_BY_SIZE, POLY_ALWAYS };
static LevelKernel level_kernel(const TailRect& tr, PolyRule poly) {
    if (poly == POLY_ALWAYS || (poly == POLY_BY_SIZE && tile_grid(tr, 128, 32).n >= 400)) return K_POLY;
    return tile_grid(tr, 64, 32).n >= 900 ? K_HV32 : K_HV16;
}
static int wide_forced() { static const int v = pbr::knob_int("PBR_BLOOM_WIDE", -1); return v; }

// One fused level (k_blur_hv / k_blur_up_poly) of nv views.  lv holds each view's input, second input (DUAL), output, output pitch and
// histogram.  MV = false: one view, the single-view kernel with view 0's pointers as its own arguments; MV: the view-table instance,
// grid (blocks, nv), whose kernel choice is the one a single view of the level gets.  The rectangles: see tail_rect.
template <int MODE, bool DUAL, int TAIL, bool MV = false>
static pbr_status launch_hv(pbr_ctx* ctx, const LevelViews& lv, uint32_t nv, uint32_t iw, uint32_t ih, uint32_t ow, uint32_t oh,
                            const uint32_t* rect, float min_log, float inv_range,
                            const uint32_t* merge_rect = nullptr, const uint32_t* buf_origin = nullptr) {
    using VS = std::conditional_t<MV, LevelViews, NoViews>;
    VS vs{};
    if constexpr (MV) vs = lv;
    TailRect tr = tail_rect(ow, oh, rect, merge_rect, buf_origin);
    // the histogram instance runs ~1024 blocks (views: over the whole batch) that each walk the same number of tiles: an uneven split
    // leaves the chip half empty for the last round, and one block per tile costs 256 contended global atomics per tile
    static const int hist_blocks = pbr::knob_int("PBR_BLOOM_HIST_BLOCKS", 1024);
    auto even_blocks = [nv](int n_tiles) { const int per = (n_tiles * (int)nv + hist_blocks - 1) / hist_blocks; return (n_tiles + per - 1) / per; };
    // every kernel of the level takes the same arguments, 512 threads and a 1-D grid over the tiles of `g` (MV: the pointer arguments are unused)
    auto launch = [&](auto kernel, const TileGrid& g, const char* label) {
        tr.tx0 = g.tx0; tr.ty0 = g.ty0;
        hipLaunchKernelGGL(kernel, dim3(TAIL == 2 ? even_blocks(g.n) : g.n, nv), dim3(512), 0, ctx->stream,
                           MV ? nullptr : lv.in[0], (int)iw, (int)ih, MV ? nullptr : lv.in2[0], MV ? nullptr : lv.out[0], (int)ow, (int)oh,
                           MV ? 0 : lv.out_pitch[0], g.tiles_x, g.n, tr, min_log, inv_range, vs, MV ? nullptr : lv.hist[0]);
        return launched(ctx, label);
    };
    // The kernel choice (level_kernel).  Only 2x-up levels have a polyphase kernel; PBR_BLOOM_WIDE=0|1 forces it off or on, and the
    // shader-order switch turns it off.
    const PolyRule poly = MODE != M_UP ? POLY_NEVER : wide_forced() >= 0 ? (wide_forced() == 1 ? POLY_ALWAYS : POLY_NEVER)
                        : ctx->bloom_shader_order ? POLY_NEVER : POLY_BY_SIZE;
    const LevelKernel k = level_kernel(tr, poly);
    if constexpr (MODE == M_UP)
        if (k == K_POLY) return launch(k_blur_up_poly<DUAL, TAIL, 32, VS>, tile_grid(tr, 128, 32), MV ? "k_blur_up_poly<views>" : "k_blur_up_poly");
    if (k == K_HV32) return launch(k_blur_hv<MODE, DUAL, TAIL, 32, 512, VS>, tile_grid(tr, 64, 32), MV ? "k_blur_hv/32<views>" : "k_blur_hv/32");
    return launch(k_blur_hv<MODE, DUAL, TAIL, 16, 512, VS>, tile_grid(tr, 64, 16), MV ? "k_blur_hv/16<views>" : "k_blur_hv/16");
}

// a fused level's view table for n views: io(i) gives view i's input, second input (DUAL; else null), output, output pitch, histogram
struct LevelIO { const pbr_half* in; const pbr_half* in2; pbr_half* out; int out_pitch; uint32_t* hist; };
template <class F>
static LevelViews level_views(uint32_t n, F io) {
    LevelViews lv{};
    for (uint32_t i = 0; i < n; i++) {
        const LevelIO v = io(i);
        lv.in[i] = v.in; lv.in2[i] = v.in2; lv.out[i] = v.out; lv.out_pitch[i] = v.out_pitch; lv.hist[i] = v.hist;
    }
    return lv;
}

// the shared-sample prefilter's rectangle table (rcs: n output rectangles sharing one destination offset / pitch)
static OutRects out_rects(const OutRect* rcs, int n) {
    OutRects rs{};
    rs.n = n; rs.ox = rcs[0].ox; rs.oy = rcs[0].oy; rs.pitch = rcs[0].pitch;
    int blocks = 0;
    for (int r = 0; r < n; r++) {
        rs.x0[r] = rcs[r].x0; rs.y0[r] = rcs[r].y0; rs.x1[r] = rcs[r].x1; rs.y1[r] = rcs[r].y1;
        rs.tiles_x[r] = (rcs[r].x1 - rcs[r].x0 + PF_TW - 1) / PF_TW;
        rs.first[r] = blocks;
        blocks += rs.tiles_x[r] * ((rcs[r].y1 - rcs[r].y0 + PF_TH - 1) / PF_TH);
    }
    rs.first[n] = blocks;
    return rs;
}

static pbr_status prefilter_launch(pbr_ctx* ctx, const pbr_half* hdr, uint32_t w, uint32_t h, uint32_t pitch,
                                   pbr_half* out, const OutRect* rcs, int n, float threshold, float knee) {
    const uint32_t ow = w >> 1, oh = h >> 1;
    const float tx = 1.0f / (float)ow, ty = 1.0f / (float)oh;   // DeferredPipeline.cpp:418
    if (exact_half(w) && exact_half(h)) {   // shared-sample kernel (bit-identical), all rectangles in one launch
        const OutRects rs = out_rects(rcs, n);
        hipLaunchKernelGGL(k_bloom_prefilter_2x<NoViews>, dim3(rs.first[n]), dim3(256), 0, ctx->stream, hdr, (int)w, (int)h, (int)pitch, NoViews{}, out, rs, threshold, knee);
        return launched(ctx, "k_bloom_prefilter_2x");
    }
    for (int r = 0; r < n; r++) {
        const uint32_t rw = (uint32_t)(rcs[r].x1 - rcs[r].x0), rh = (uint32_t)(rcs[r].y1 - rcs[r].y0);
        dim3 grid((rw + 63) / 64, (rh + 3) / 4);
        hipLaunchKernelGGL(k_bloom_prefilter, grid, dim3(64, 4), 0, ctx->stream, hdr, (int)w, (int)h, (int)pitch, out, rcs[r], tx, ty, threshold, knee);
        pbr_status st = launched(ctx, "k_bloom_prefilter");
        if (st) return st;
    }
    return PBR_OK;
}

// ---- checks with more than one reason, or more than one caller: what is wrong (nullptr: nothing); the caller refuses under its own name (PBR_CHECK)
// prefilter: output rectangle q = {x, y, w, h} inside the half-res image, and inside the destination's pitch when placed at column out_x
static const char* prefilter_rect_fault(const uint32_t q[4], uint32_t w, uint32_t h, uint32_t out_x, uint32_t out_pitch) {
    if (!(q[2] >= 1 && q[3] >= 1 && q[0] + q[2] <= (w >> 1) && q[1] + q[3] <= (h >> 1))) return "rect outside the half-res image";
    return out_pitch >= out_x + q[0] + q[2] ? nullptr : "rect does not fit the output pitch";
}
// chain: every one of the five mips >= 1 texel (BloomStep < CalculateMaxMipLevels, DeferredPipeline.cpp:343), sides <= 65535, pitch >= w
static const char* chain_size_fault(uint32_t w, uint32_t h, uint32_t pitch) {
    if (!((w >> (PBR_BLOOM_MIPS - 1)) >= 1 && (h >> (PBR_BLOOM_MIPS - 1)) >= 1)) return "image too small for 5 mips";
    return w <= 65535 && h <= 65535 && pitch >= w ? nullptr : "bad size";
}

// ---------------------------------------------------------------- C ABI: the staged passes
extern "C" {

pbr_status pbr_bloom_prefilter(pbr_ctx* ctx, const pbr_bloom_prefilter_desc* d) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, d, "pbr_bloom_prefilter: null descriptor");
    PBR_REQUIRE(ctx, d->reserved == 0, "pbr_bloom_prefilter: reserved must be 0");
    PBR_REQUIRE(ctx, d->hdr && d->out, "pbr_bloom_prefilter: null pointer");
    // no rectangles: the whole half-res image into a dense plane, as the one rectangle it is
    const uint32_t w = d->w, h = d->h, whole[1][4] = {{0, 0, w >> 1, h >> 1}};
    const bool dense = !d->rects && d->n_rects == 0;
    const uint32_t (*rects)[4] = dense ? whole : d->rects;
    const uint32_t n = dense ? 1 : d->n_rects, out_pitch = dense ? w >> 1 : d->out_pitch;
    PBR_REQUIRE(ctx, rects && n >= 1 && n <= (uint32_t)PF_MAX_RECTS, "pbr_bloom_prefilter: null pointer / 1 .. 5 rectangles");
    PBR_REQUIRE(ctx, (w >> 1) >= 1 && (h >> 1) >= 1 && w <= 65535 && h <= 65535 && d->pitch >= w, "pbr_bloom_prefilter: bad size");
    PBR_REQUIRE(ctx, !dense || (!d->out_pitch && !d->out_x && !d->out_y), "pbr_bloom_prefilter: out_pitch, out_x and out_y must be 0 without rects");
    PBR_REQUIRE(ctx, out_pitch <= 65535 && d->out_y <= 65535, "pbr_bloom_prefilter: bad size");
    OutRect rcs[PF_MAX_RECTS];
    for (uint32_t r = 0; r < n; r++) {
        const uint32_t* q = rects[r];
        PBR_CHECK(ctx, "pbr_bloom_prefilter", prefilter_rect_fault(q, w, h, d->out_x, out_pitch));
        rcs[r] = OutRect{(int)q[0], (int)q[1], (int)(q[0] + q[2]), (int)(q[1] + q[3]), (int)d->out_x, (int)d->out_y, (int)out_pitch};
    }
    return prefilter_launch(ctx, d->hdr, w, h, d->pitch, d->out, rcs, (int)n, d->threshold, d->knee);
}

pbr_status pbr_blur_h(pbr_ctx* ctx, const pbr_half* in, uint32_t iw, uint32_t ih, pbr_half* out, uint32_t ow, uint32_t oh) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, in && out, "pbr_blur_h: null pointer");
    PBR_REQUIRE(ctx, iw && ih && ow && oh && iw <= 65535 && ih <= 65535 && ow <= 65535 && oh <= 65535, "pbr_blur_h: bad size");
    return launch_blur_h<false>(ctx, in, iw, ih, nullptr, 0, 0, out, ow, oh);
}

pbr_status pbr_blur_v(pbr_ctx* ctx, const pbr_half* in, uint32_t iw, uint32_t ih, pbr_half* out, uint32_t ow, uint32_t oh) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, in && out, "pbr_blur_v: null pointer");
    PBR_REQUIRE(ctx, iw && ih && ow && oh && iw <= 65535 && ih <= 65535 && ow <= 65535 && oh <= 65535, "pbr_blur_v: bad size");
    const float tx = 1.0f / (float)ow, ty = 1.0f / (float)oh;
    dim3 grid((ow + VT_W - 1) / VT_W, (oh + VT_R - 1) / VT_R);
    hipLaunchKernelGGL(k_blur_v, grid, dim3(VT_W, 4), 0, ctx->stream, in, (int)iw, (int)ih, out, (int)ow, (int)oh, tx, ty);
    return launched(ctx, "k_blur_v");
}

pbr_status pbr_bloom_upsample_add(pbr_ctx* ctx, const pbr_half* upper, uint32_t uw, uint32_t uh,
                                  const pbr_half* lower, uint32_t lw, uint32_t lh, pbr_half* out) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, upper && lower && out, "pbr_bloom_upsample_add: null pointer");
    PBR_REQUIRE(ctx, uw && uh && lw && lh && uw <= 65535 && uh <= 65535, "pbr_bloom_upsample_add: bad size");
    return launch_blur_h<true>(ctx, lower, lw, lh, upper, uw, uh, out, uw, uh);   // bloom_upsample_add.hlsl: lower first, then upper
}

pbr_status pbr_bloom_merge(pbr_ctx* ctx, pbr_half* hdr, uint32_t pitch, const pbr_half* in, uint32_t w, uint32_t h) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, hdr && in, "pbr_bloom_merge: null pointer");
    PBR_REQUIRE(ctx, w && h && w <= 65535 && h <= 65535 && pitch >= w, "pbr_bloom_merge: bad size");
    dim3 grid((w + 255) / 256, h);
    hipLaunchKernelGGL(k_bloom_merge, grid, dim3(256), 0, ctx->stream, hdr, (int)pitch, in, (int)w, (int)h);
    return launched(ctx, "k_bloom_merge");
}

pbr_status pbr_bloom_up_level(pbr_ctx* ctx, const pbr_half* upper, const pbr_half* lower, uint32_t lw, uint32_t lh,
                              pbr_half* out, uint32_t ow, uint32_t oh) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, lower && out && out != lower && out != upper, "pbr_bloom_up_level: null pointer / out aliases an input");
    PBR_REQUIRE(ctx, lw >= 1 && lh >= 1 && ow == 2 * lw && oh == 2 * lh && exact_half(ow) && exact_half(oh), "pbr_bloom_up_level: out must be exactly twice lower, even, <= 8192");
    const LevelViews lv = level_views(1, [&](uint32_t) { return LevelIO{lower, upper, out, (int)ow, nullptr}; });
    if (upper) return launch_hv<M_UP, true, 0>(ctx, lv, 1, lw, lh, ow, oh, nullptr, 0.0f, 0.0f);
    return launch_hv<M_UP, false, 0>(ctx, lv, 1, lw, lh, ow, oh, nullptr, 0.0f, 0.0f);
}

}  // extern "C"

// ---------------------------------------------------------------- schedule
// the staged chain's last two dispatches + the histogram: k_blur_v_merge on level 0 of chain B
static pbr_status bloom_final(pbr_ctx* ctx, const pbr_half* b0, pbr_half* hdr, uint32_t w, uint32_t h, uint32_t pitch,
                              const uint32_t* hist_rect, float min_log, float inv_range, uint32_t* hist256) {
    const float tx = 1.0f / (float)w, ty = 1.0f / (float)h;
    const int tiles_x = (int)((w + VT_W - 1) / VT_W), tiles_y = (int)((h + VT_R - 1) / VT_R);
    int blocks = tiles_x * tiles_y;
    if (blocks > 1280) blocks = 1280;   // 5 blocks (24.6 + 4 KB LDS each) resident per CU x 256 CUs: one full wave of persistent blocks
    if (hist256) {
        hipLaunchKernelGGL(k_blur_v_merge<true>, dim3(blocks), dim3(VT_W, 4), 0, ctx->stream, b0, (int)w, (int)h, tx, ty, hdr, (int)pitch, tiles_x, tiles_y,
                           (int)hist_rect[0], (int)hist_rect[1], (int)(hist_rect[0] + hist_rect[2]), (int)(hist_rect[1] + hist_rect[3]), min_log, inv_range, hist256);
    } else {
        hipLaunchKernelGGL(k_blur_v_merge<false>, dim3(blocks), dim3(VT_W, 4), 0, ctx->stream, b0, (int)w, (int)h, tx, ty, hdr, (int)pitch, tiles_x, tiles_y,
                           0, 0, 0, 0, 0.0f, 0.0f, (uint32_t*)nullptr);
    }
    return launched(ctx, "k_blur_v_merge");
}

// Rectangles {x, y, w, h} of the up-levels 1 .. PBR_BLOOM_MIPS - 1 (level coordinates) that the finished image inside merge0 depends
// on.  Level 1's result is read by the merge within merge0 / 2 +- 3 texels (nine taps one level-0 texel apart + the bilinear
// footprint); level l's up-pass reads the level below within +- 4 of its own taps, halved, + the bilinear footprint.  So the
// rectangle shrinks towards merge0 / 2^l as the remaining filter support does.  Margins are rounded up: a superset costs a tile at most.
static void up_pass_rects(const uint32_t merge0[4], uint32_t w, uint32_t h, uint32_t need[PBR_BLOOM_MIPS][4]) {
    int x0 = (int)merge0[0], y0 = (int)merge0[1], x1 = (int)(merge0[0] + merge0[2]), y1 = (int)(merge0[1] + merge0[3]);
    for (uint32_t l = 1; l < PBR_BLOOM_MIPS; l++) {
        const int lw = (int)(w >> l), lh = (int)(h >> l);
        x0 = (x0 - 4) / 2 - 2; y0 = (y0 - 4) / 2 - 2; x1 = (x1 + 4 + 1) / 2 + 2; y1 = (y1 + 4 + 1) / 2 + 2;   // (C division of a negative numerator rounds towards 0: clipped below anyway)
        x0 = x0 < 0 ? 0 : x0; y0 = y0 < 0 ? 0 : y0; x1 = x1 > lw ? lw : x1; y1 = y1 > lh ? lh : y1;
        need[l][0] = (uint32_t)x0; need[l][1] = (uint32_t)y0; need[l][2] = (uint32_t)(x1 - x0); need[l][3] = (uint32_t)(y1 - y0);
    }
}

// One view of a bloom pass: its HDR target (w x h, pitch), the two chains and its histogram (null: no histogram)
struct BloomView { pbr_half* hdr; uint32_t pitch; pbr_half* A; pbr_half* B; uint32_t* hist; };

// BloomPass::Execute (DeferredPipeline.cpp:400-570; schedule comment :379-399) + the histogram dispatch of AutoExposurePass::Execute
// (DeferredPipeline.cpp:276-298) on n views of one size: the prefilter into level 1 of chain A (if `prefilter`), the three downsample
// pairs, the three upsample-add pairs and the level-0 H + V + merge (+ histogram of hist_rect).  MV = false: one view on the single-view
// kernels; MV: up to PBR_MAX_VIEWS views, every fused kernel in one launch with the view table (grid (blocks of one view, views)).
//
// Per level pair: where level l+1 is exactly half of level l (and both fit the fast path's size limit) the H and V pass run as one
// kernel and the H result (chain B of the reference schedule) is never written; elsewhere the two staged kernels run, once per view.
// 1920x1080, for instance, is exact down to 240x135 and staged for 135 -> 67.  Fused up-levels write chain B (a block must not
// overwrite what its neighbours still read), so `res_in_b` tracks where the finished level below lives.  Chain contents after the call
// are scratch.
//
// merge0 (one view, exact level 0 only): the rectangle {x, y, w, h} of level 0 to merge; origin: its level coordinates of hdr[0].  The
// up-pass of level l is then run only on the tiles of level l inside up_pass_rects' rectangle (a tiled frame's bloom works on the
// tile +- 256 px, but only the DOWN-pass needs that apron in full: SURVEY 8e's "cheaper apron").  Whole tiles are computed, so every
// texel inside the rectangles is what the SAME kernel computes on the whole level: the merged interior is bit-identical to the full
// up-pass where both select the same kernels.  launch_hv chooses by the tiles of the rectangle — the work the launch really has —
// so a level can take k_blur_hv on its rectangle where the whole level takes k_blur_up_poly (level 1 of a 2432 x 2672 extended tile;
// tests/bloom_truth.py up_kernel says where); then both results lie inside the pyramid's float64 interval and differ by at most one
// half step per stage (tests/test_gpu_bloom_tiled_truth.py).  Texels of the up-levels outside the rectangles are left as they were.
template <bool MV>
static pbr_status bloom_pass(pbr_ctx* ctx, const BloomView* v, uint32_t n, uint32_t w, uint32_t h, bool prefilter, float threshold, float knee,
                             const uint32_t* hist_rect, float min_log, float inv_range, const uint32_t* merge0 = nullptr, const uint32_t* origin = nullptr) {
    auto W = [&](uint32_t l) { return w >> l; };
    auto H = [&](uint32_t l) { return h >> l; };
    auto off = [&](uint32_t l) { return (size_t)4 * pbr_bloom_level_offset(w, h, l); };
    auto exact = [&](uint32_t l) { return exact_half(W(l)) && exact_half(H(l)); };
    pbr_status r;
    if (prefilter) {   // hdr -> level 1 of chain A
        const OutRect whole{0, 0, (int)W(1), (int)H(1), 0, 0, (int)W(1)};
        if (MV && exact(0)) {
            PrefilterViews pv{};
            for (uint32_t i = 0; i < n; i++) { pv.hdr[i] = v[i].hdr; pv.out[i] = v[i].A + off(1); pv.pitch[i] = (int)v[i].pitch; }
            const OutRects rs = out_rects(&whole, 1);
            hipLaunchKernelGGL(k_bloom_prefilter_2x<PrefilterViews>, dim3(rs.first[1], n), dim3(256), 0, ctx->stream,
                               nullptr, (int)w, (int)h, 0, pv, nullptr, rs, threshold, knee);
            if ((r = launched(ctx, "k_bloom_prefilter_2x<views>"))) return r;
        } else {
            for (uint32_t i = 0; i < n; i++)
                if ((r = prefilter_launch(ctx, v[i].hdr, w, h, v[i].pitch, v[i].A + off(1), &whole, 1, threshold, knee))) return r;
        }
    }
    // The small end in one launch (k_bloom_small_end; PBR_BLOOM_SMALL_END = 0 | 1 | 2 levels folded): one view of whole frames whose
    // levels 1 - 3 are exact halves, and whose folded up-passes would each take k_blur_hv/16, the kernel it restates bit for bit.
    // Depth 2 skips the down pass 3 -> 4 and level 3's up-pass, and level 2's up-pass reads chain A levels 3 and 2; depth 1 skips
    // the down pass alone.  Chain A level 4 (and chain B level 3) are then not written.  The product takes depth 2 (the measured keep:
    // EXPERIMENTS.md), and today's launches where level 2 is large enough for another kernel.
    static const int small_end_knob = pbr::knob_int("PBR_BLOOM_SMALL_END", 2);
    // the whole level's kernel as shipped is k_blur_hv/16: whatever the shader-order switch says, and PBR_BLOOM_WIDE=0 counts as unset
    auto takes_hv16 = [&](uint32_t l) {
        return level_kernel(tail_rect(W(l), H(l), nullptr, nullptr, nullptr), wide_forced() == 1 ? POLY_ALWAYS : POLY_BY_SIZE) == K_HV16;
    };
    int small_end = 0;
    if (!MV && n == 1 && merge0 == nullptr && PBR_BLOOM_STEP == 3 && exact(1) && exact(2) && exact(3) && takes_hv16(3)) {
        small_end = small_end_knob == 2 ? (takes_hv16(2) ? 2 : 0) : (small_end_knob == 1 ? 1 : 0);
    }
    auto launch_small_end = [&](uint32_t l) {   // the up-pass of level l (3: depth 1; 2: depth 2) into chain B
        const int tiles_x = (int)((W(l) + 63) / 64), tiles = tiles_x * (int)((H(l) + 15) / 16);
        if (l == 3) hipLaunchKernelGGL(k_bloom_small_end<1>, dim3(tiles), dim3(small_end::NT), 0, ctx->stream, (const pbr_half*)(v[0].A + off(3)), (int)W(3), (int)H(3),
                                       (const pbr_half*)nullptr, v[0].B + off(3), (int)W(3), (int)H(3), tiles_x);
        else hipLaunchKernelGGL(k_bloom_small_end<2>, dim3(tiles), dim3(small_end::NT), 0, ctx->stream, (const pbr_half*)(v[0].A + off(3)), (int)W(3), (int)H(3),
                                (const pbr_half*)(v[0].A + off(2)), v[0].B + off(2), (int)W(2), (int)H(2), tiles_x);
        return launched(ctx, l == 3 ? "k_bloom_small_end/1" : "k_bloom_small_end/2");
    };
    for (uint32_t k = 0; k < PBR_BLOOM_STEP; k++) {   // downsample
        const uint32_t up = k + 1, lo = k + 2;
        if (small_end && lo == PBR_BLOOM_MIPS - 1) break;   // level 4 is computed where it is used
        if (exact(up)) {
            const LevelViews lv = level_views(n, [&](uint32_t i) { return LevelIO{v[i].A + off(up), nullptr, v[i].A + off(lo), (int)W(lo), nullptr}; });
            if ((r = launch_hv<M_DOWN, false, 0, MV>(ctx, lv, n, W(up), H(up), W(lo), H(lo), nullptr, 0.0f, 0.0f))) return r;
        } else {
            for (uint32_t i = 0; i < n; i++) {
                if ((r = pbr_blur_h(ctx, v[i].A + off(up), W(up), H(up), v[i].B + off(lo), W(lo), H(lo)))) return r;
                if ((r = pbr_blur_v(ctx, v[i].B + off(lo), W(lo), H(lo), v[i].A + off(lo), W(lo), H(lo)))) return r;
            }
        }
    }
    uint32_t need[PBR_BLOOM_MIPS][4];
    static const bool shrink = pbr::knob_int("PBR_BLOOM_SHRINK", 1) != 0;
    const bool use_need = merge0 != nullptr && shrink;
    if (use_need) up_pass_rects(merge0, w, h, need);
    bool res_in_b = false;
    uint32_t res_level = PBR_BLOOM_MIPS - 1;
    auto res = [&](uint32_t i) { return (const pbr_half*)(res_in_b ? v[i].B : v[i].A) + off(res_level); };
    for (int k = PBR_BLOOM_STEP - 1; k >= 0; k--) {   // upsample: V(H(lower) + H(upper))
        const uint32_t up = (uint32_t)k + 1;
        if (small_end && up + (uint32_t)small_end >= PBR_BLOOM_MIPS - 1) {   // depth 1: level 3; depth 2: level 3 (nothing to launch) and level 2
            if (up + (uint32_t)small_end == PBR_BLOOM_MIPS - 1 && (r = launch_small_end(up))) return r;
            res_in_b = true;
        } else if (exact(up)) {
            const LevelViews lv = level_views(n, [&](uint32_t i) { return LevelIO{res(i), v[i].A + off(up), v[i].B + off(up), (int)W(up), nullptr}; });
            if ((r = launch_hv<M_UP, true, 0, MV>(ctx, lv, n, W(up + 1), H(up + 1), W(up), H(up), nullptr, 0.0f, 0.0f,
                                                  use_need ? need[up] : nullptr))) return r;
            res_in_b = true;
        } else {
            for (uint32_t i = 0; i < n; i++) {
                if ((r = pbr_bloom_upsample_add(ctx, v[i].A + off(up), W(up), H(up), res(i), W(up + 1), H(up + 1), v[i].B + off(up)))) return r;
                if ((r = pbr_blur_v(ctx, v[i].B + off(up), W(up), H(up), v[i].A + off(up), W(up), H(up)))) return r;
            }
            res_in_b = false;
        }
        res_level = up;
    }
    if (exact(0)) {   // H + V + merge (+ histogram) in one kernel
        const LevelViews lv = level_views(n, [&](uint32_t i) { return LevelIO{res(i), nullptr, v[i].hdr, (int)v[i].pitch, v[i].hist}; });
        if constexpr (!MV)
            if (!v[0].hist) return launch_hv<M_UP, false, 1>(ctx, lv, 1, w >> 1, h >> 1, w, h, nullptr, 0.0f, 0.0f, merge0, origin);
        return launch_hv<M_UP, false, 2, MV>(ctx, lv, n, w >> 1, h >> 1, w, h, hist_rect, min_log, inv_range, merge0, origin);
    }
    for (uint32_t i = 0; i < n; i++) {
        if ((r = pbr_blur_h(ctx, res(i), w >> 1, h >> 1, v[i].B, w, h))) return r;   // level 0 of chain B
        // A0 = V(B0); S += A0 [; histogram(S)] in one pass — chain A level 0 is not materialised
        if ((r = bloom_final(ctx, v[i].B, v[i].hdr, w, h, v[i].pitch, hist_rect, min_log, inv_range, v[i].hist))) return r;
    }
    return PBR_OK;
}

// ---------------------------------------------------------------- C ABI: the chain
extern "C" {

// Whole-image form (hdr_rect == NULL): BloomPass::Execute, with hist_rect + hist256 followed by AutoExposurePass::Execute's histogram
// dispatch on hist_rect.  Tiled form, the multi-GPU halo path (SURVEY 8e option 2): BloomPass::Execute minus the prefilter on the
// extended rectangle E (w x h) of a tile, merged (+ counted) inside merge_rect only; hdr covers hdr_rect of E (include/pbr_hip.h).
pbr_status pbr_bloom(pbr_ctx* ctx, const pbr_bloom_desc* d) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, d, "pbr_bloom: null descriptor");
    PBR_REQUIRE(ctx, d->reserved == 0, "pbr_bloom: reserved must be 0");
    const BloomView v{d->hdr, d->hdr_pitch, d->chain_a, d->chain_b, d->hist256};
    const uint32_t w = d->w, h = d->h;
    if (!d->hdr_rect) {
        const uint32_t* rect = d->hist_rect;
        PBR_REQUIRE(ctx, !d->merge_rect, "pbr_bloom: merge_rect without hdr_rect");
        PBR_REQUIRE(ctx, !rect || d->hist256, "pbr_bloom: hist_rect without hist256");
        PBR_REQUIRE(ctx, rect || !d->hist256, "pbr_bloom: hist256 without hist_rect");
        PBR_REQUIRE(ctx, !rect || (rect[2] >= 1 && rect[3] >= 1 && rect[0] + rect[2] <= w && rect[1] + rect[3] <= h), "pbr_bloom: rect outside the image");
        PBR_REQUIRE(ctx, v.hdr && v.A && v.B, "pbr_bloom: null pointer");
        PBR_CHECK(ctx, "pbr_bloom", chain_size_fault(w, h, v.pitch));
        return bloom_pass<false>(ctx, &v, 1, w, h, true, d->threshold, d->knee, rect, d->min_log, d->inv_range);
    }
    const uint32_t *hdr_rect = d->hdr_rect, *merge_rect = d->merge_rect;
    PBR_REQUIRE(ctx, !d->hist_rect, "pbr_bloom: hist_rect in the tiled form (the histogram counts merge_rect)");
    PBR_REQUIRE(ctx, v.hdr && v.A && v.B && merge_rect, "pbr_bloom: null pointer");
    PBR_REQUIRE(ctx, !chain_size_fault(w, h, w), "pbr_bloom: bad size");   // (the pitch is hdr_rect's: below)
    PBR_REQUIRE(ctx, hdr_rect[2] >= 1 && hdr_rect[3] >= 1 && hdr_rect[0] + hdr_rect[2] <= w && hdr_rect[1] + hdr_rect[3] <= h && v.pitch >= hdr_rect[2],
                "pbr_bloom: hdr_rect outside the extended tile");
    PBR_REQUIRE(ctx, merge_rect[2] >= 1 && merge_rect[3] >= 1 && merge_rect[0] >= hdr_rect[0] && merge_rect[1] >= hdr_rect[1] &&
                     merge_rect[0] + merge_rect[2] <= hdr_rect[0] + hdr_rect[2] && merge_rect[1] + merge_rect[3] <= hdr_rect[1] + hdr_rect[3],
                "pbr_bloom: merge_rect outside hdr_rect");
    if (!exact_half(w) || !exact_half(h))
        return pbr::fail(ctx, PBR_ERR_UNSUPPORTED, "pbr_bloom: the extended tile must be even and <= 8192 on a side");
    return bloom_pass<false>(ctx, &v, 1, w, h, false, 0.0f, 0.0f, merge_rect, d->min_log, d->inv_range, merge_rect, hdr_rect);
}

// pbr_bloom's whole-image form with the whole-frame histogram, for up to PBR_MAX_VIEWS frames of one size: every level takes the kernel a
// single view of that size takes (bloom_pass); fused levels run all views in one launch, staged levels (not an exact half, e.g. 1920x1080 from level 3 down) run the
// single-view staged kernels once per view.
pbr_status pbr_bloom_histogram_views(pbr_ctx* ctx, const pbr_view* views, uint32_t n, uint32_t w, uint32_t h,
                                     float threshold, float knee, float min_log, float inv_range) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, views_count_ok(views, n), "pbr_bloom_histogram_views: need 1 .. PBR_MAX_VIEWS views");
    PBR_CHECK(ctx, "pbr_bloom_histogram_views", chain_size_fault(w, h, w));   // (each view's pitch: below)
    BloomView bv[PBR_MAX_VIEWS];
    for (uint32_t i = 0; i < n; i++) {
        const pbr_view& v = views[i];
        PBR_REQUIRE(ctx, v.hdr && v.chain_a && v.chain_b && v.hist256, "pbr_bloom_histogram_views: null pointer");
        PBR_REQUIRE(ctx, v.hdr_pitch >= w, "pbr_bloom_histogram_views: bad size");
        bv[i] = BloomView{v.hdr, v.hdr_pitch, v.chain_a, v.chain_b, v.hist256};
    }
    const size_t chain_bytes = pbr_bloom_chain_texels(w, h) * 8u;
    PBR_REQUIRE(ctx, views_disjoint(views, n, 4, [&](const pbr_view& v, int k, uintptr_t& lo, uintptr_t& hi) {
                    if (k == 0) { lo = addr(v.hdr); hi = lo + ((size_t)v.hdr_pitch * (h - 1) + w) * 8u; }
                    else if (k == 1) { lo = addr(v.chain_a); hi = lo + chain_bytes; }
                    else if (k == 2) { lo = addr(v.chain_b); hi = lo + chain_bytes; }
                    else { lo = addr(v.hist256); hi = lo + PBR_HISTOGRAM_BINS * sizeof(uint32_t); } }),
                "pbr_bloom_histogram_views: two views share an HDR target, a bloom chain or a histogram");
    const uint32_t rect[4] = {0, 0, w, h};
    return bloom_pass<true>(ctx, bv, n, w, h, true, threshold, knee, rect, min_log, inv_range);
}

}  // extern "C"
