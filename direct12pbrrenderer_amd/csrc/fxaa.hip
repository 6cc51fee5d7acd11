// fxaa.hip — the anti-aliasing pass on the tone-mapped RGBA8 target (include/pbr_hip.h, "Anti-aliasing"): an edge filter of FXAA's
// structure under an all-integer rule that is this project's own (the reference has no anti-aliasing).  The rule for one pixel is
// fxaa_pixel.hpp, which tools/fxaa_hostcheck.cpp compiles for the host; tests/fxaa_ref.py restates it, and the kernel is bit-identical
// to the restatement on every pixel.
//   k_fxaa<Batch>      block = 256 lanes = a 64 x 16 tile of one image, lane = four pixels of a row (one 16-byte load, one 16-byte
//                        store where pointer and pitch allow; 4-byte accesses otherwise and at the right border).  The block stages its
//                        tile and a one-pixel ring in LDS, as pixels and as luma (clamped at the image border, like every read of the
//                        rule), and classifies its pixels from the luma plane.  An edge pixel's walk reads LDS inside the staged
//                        18 x 66 and global memory beyond it: lines of the neighbouring blocks' tiles, which sit in L2.
//                        The block appends its edge pixels to an LDS list and all lanes work through the list densely, so a wave
//                        with six edge pixels does not run the walk with six lanes of 64; the results go through an LDS tile back to
//                        the lanes that store them.  (The plain form, each lane resolving its own pixels, took 2.5 x as long on a
//                        rendered 1440 x 960 frame: EXPERIMENTS.md, profiles/fxaa_forms_ab.txt.)
//                        Batch: the image index is blockIdx.z, the image table arrives by value in the kernel arguments.
// Integers only: no -ffp-contract flag matters here.
#include <cstdint>

#include "pbr_internal.hpp"
#include "fxaa_pixel.hpp"

namespace {

constexpr int TILE_W = 64, TILE_H = 16;                 // pixels of a block
constexpr int STAGE_W = TILE_W + 2, STAGE_H = TILE_H + 2;
constexpr int LDS_PITCH = 72, LDS_X0 = 3;               // the ring's first column sits at 3, so the tile's first at 4: 16-byte aligned rows
constexpr int RING = 2 * STAGE_W + 2 * TILE_H;          // 164 pixels around the tile
static_assert(RING <= 256 && TILE_W * TILE_H == 4 * 256 && (LDS_PITCH * 4) % 16 == 0 && LDS_X0 + STAGE_W <= LDS_PITCH, "k_fxaa's tile");

template <bool Batch>
struct FxaaArgs {
    uint32_t w, h;
    pbr_fxaa_image img[Batch ? PBR_MAX_VIEWS : 1];
};

// the rule's fetcher inside a block: the staged 18 x 66 from LDS, everything else from the image
struct TileFetch {
    const uint32_t* pix;        // LDS, [STAGE_H][LDS_PITCH]
    const uint32_t* lum;
    int sx0, sy0;               // image coordinates of the stage's first pixel (the tile's origin minus one)
    const uint32_t* src;
    uint32_t pitch;
    __device__ __forceinline__ bool staged(int x, int y, int& at) const {
        const int lx = x - sx0, ly = y - sy0;
        at = ly * LDS_PITCH + LDS_X0 + lx;
        return (unsigned)lx < (unsigned)STAGE_W && (unsigned)ly < (unsigned)STAGE_H;
    }
    __device__ __forceinline__ uint32_t rgba(int x, int y) const {
        int at;
        return staged(x, y, at) ? pix[at] : src[(size_t)y * pitch + (size_t)x];
    }
    __device__ __forceinline__ int luma(int x, int y) const {
        int at;
        return staged(x, y, at) ? (int)lum[at] : fxaa::luma_of(src[(size_t)y * pitch + (size_t)x]);
    }
};

template <bool Batch>
__global__ __launch_bounds__(256) void k_fxaa(const FxaaArgs<Batch> A) {
    __shared__ __attribute__((aligned(16))) uint32_t s_pix[STAGE_H * LDS_PITCH];
    __shared__ __attribute__((aligned(16))) uint32_t s_lum[STAGE_H * LDS_PITCH];
    const pbr_fxaa_image I = A.img[Batch ? blockIdx.z : 0];
    const int w = (int)A.w, h = (int)A.h;
    const int t = (int)threadIdx.x, row = t >> 4, col = (t & 15) * 4;
    const int tx0 = (int)blockIdx.x * TILE_W, ty0 = (int)blockIdx.y * TILE_H;
    const int gx = tx0 + col, gy = ty0 + row;
    const bool src_vec = (((uintptr_t)I.src | ((uintptr_t)I.src_pitch * 4u)) & 15u) == 0;
    const bool dst_vec = (((uintptr_t)I.dst | ((uintptr_t)I.dst_pitch * 4u)) & 15u) == 0;

    // ---- stage: the lane's four pixels (clamped into the image where the tile hangs over its border), then the ring
    uint32_t v[4];
    {
        const int cy = fxaa::imin(gy, h - 1);
        const uint32_t* line = I.src + (size_t)cy * I.src_pitch;
        if (src_vec && gx + 3 < w) {
            const uint4 q = *reinterpret_cast<const uint4*>(line + gx);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = line[fxaa::imin(gx + j, w - 1)];
        }
        const int at = (row + 1) * LDS_PITCH + LDS_X0 + 1 + col;
        *reinterpret_cast<uint4*>(&s_pix[at]) = make_uint4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<uint4*>(&s_lum[at]) = make_uint4((uint32_t)fxaa::luma_of(v[0]), (uint32_t)fxaa::luma_of(v[1]),
                                                           (uint32_t)fxaa::luma_of(v[2]), (uint32_t)fxaa::luma_of(v[3]));
    }
    if (t < RING) {
        int lx, ly;
        if (t < STAGE_W)                    { lx = t;               ly = 0; }
        else if (t < 2 * STAGE_W)           { lx = t - STAGE_W;     ly = STAGE_H - 1; }
        else if (t < 2 * STAGE_W + TILE_H)  { lx = 0;               ly = 1 + t - 2 * STAGE_W; }
        else                                { lx = STAGE_W - 1;     ly = 1 + t - 2 * STAGE_W - TILE_H; }
        const int x = fxaa::clampi(tx0 - 1 + lx, w - 1), y = fxaa::clampi(ty0 - 1 + ly, h - 1);
        const uint32_t p = I.src[(size_t)y * I.src_pitch + (size_t)x];
        s_pix[ly * LDS_PITCH + LDS_X0 + lx] = p;
        s_lum[ly * LDS_PITCH + LDS_X0 + lx] = (uint32_t)fxaa::luma_of(p);
    }
    __syncthreads();

    // ---- classify the lane's pixels that lie inside the image
    const TileFetch f{s_pix, s_lum, tx0 - 1, ty0 - 1, I.src, I.src_pitch};
    uint32_t edges = 0;
    if (gy < h) {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (gx + j < w && fxaa::is_edge(f, gx + j, gy, w, h)) edges |= 1u << j;
    }

    // ---- resolve the edge pixels: the block's list (in no particular order: every entry is resolved on its own), all lanes through it
    __shared__ uint32_t s_count;
    __shared__ uint16_t s_list[TILE_W * TILE_H];
    __shared__ uint32_t s_out[TILE_W * TILE_H];
    if (t == 0) s_count = 0;
    __syncthreads();
    if (edges) {
        uint32_t at = atomicAdd(&s_count, (uint32_t)__builtin_popcount(edges));
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (edges >> j & 1u) s_list[at++] = (uint16_t)(row * TILE_W + col + j);
    }
    __syncthreads();
    const uint32_t n = s_count;                          // <= TILE_W * TILE_H: one entry per pixel of the tile at most
    for (uint32_t i = (uint32_t)t; i < n; i += 256u) {
        const uint32_t px = s_list[i];
        s_out[px] = fxaa::filter_edge(f, tx0 + (int)(px & (TILE_W - 1)), ty0 + (int)(px / TILE_W), w, h);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (edges >> j & 1u) v[j] = s_out[row * TILE_W + col + j];

    // ---- store
    if (gy < h && gx < w) {
        uint32_t* line = I.dst + (size_t)gy * I.dst_pitch;
        if (dst_vec && gx + 3 < w) {
            *reinterpret_cast<uint4*>(line + gx) = make_uint4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (gx + j < w) line[gx + j] = v[j];
        }
    }
}

// [begin, end) in bytes of an image's pixels: its last row ends after w pixels, not after a pitch
void image_range(const void* p, uint32_t w, uint32_t h, uint32_t pitch, uintptr_t& lo, uintptr_t& hi) {
    lo = pbr::addr(p);
    hi = lo + 4u * ((size_t)(h - 1u) * pitch + w);
}

const char* fxaa_refusal(const pbr_fxaa_image* images, uint32_t n, uint32_t w, uint32_t h) {
    if (w == 0 || h == 0) return "an empty image";
    if (w > 65535u || h > 65535u) return "an image of more than 65535 pixels on a side";
    for (uint32_t i = 0; i < n; i++) {
        if (!images[i].src || !images[i].dst) return "null pointer";
        if (images[i].src_pitch < w || images[i].dst_pitch < w) return "a pitch below w";
        if ((pbr::addr(images[i].src) | pbr::addr(images[i].dst)) & 3u) return "an image not aligned to its 4-byte pixels";
    }
    // the filter cannot run in place, and a batch's images are filtered side by side: no dst inside any src or another dst
    for (uint32_t i = 0; i < n; i++) {
        uintptr_t d0, d1, o0, o1;
        image_range(images[i].dst, w, h, images[i].dst_pitch, d0, d1);
        for (uint32_t j = 0; j < n; j++) {
            image_range(images[j].src, w, h, images[j].src_pitch, o0, o1);
            if (d0 < o1 && o0 < d1) return "a destination overlaps a source";
            if (j <= i) continue;
            image_range(images[j].dst, w, h, images[j].dst_pitch, o0, o1);
            if (d0 < o1 && o0 < d1) return "two destinations overlap";
        }
    }
    return nullptr;
}

template <bool Batch>
void launch_fxaa(pbr_ctx* ctx, const FxaaArgs<Batch>& A, uint32_t n) {
    const dim3 grid((A.w + TILE_W - 1) / TILE_W, (A.h + TILE_H - 1) / TILE_H, n), block(256);
    hipLaunchKernelGGL((k_fxaa<Batch>), grid, block, 0, ctx->stream, A);
}

}  // namespace

extern "C" {

pbr_status pbr_fxaa(pbr_ctx* ctx, const uint32_t* src, uint32_t w, uint32_t h, uint32_t src_pitch, uint32_t* dst, uint32_t dst_pitch) {
    if (!ctx) return PBR_ERR_INVALID;
    FxaaArgs<false> A;
    A.w = w;
    A.h = h;
    A.img[0] = pbr_fxaa_image{src, src_pitch, dst, dst_pitch};
    PBR_CHECK(ctx, "pbr_fxaa", fxaa_refusal(A.img, 1, w, h));
    launch_fxaa<false>(ctx, A, 1);
    return pbr::launched(ctx, "k_fxaa");
}

pbr_status pbr_fxaa_batch(pbr_ctx* ctx, const pbr_fxaa_image* images, uint32_t n, uint32_t w, uint32_t h) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, images != nullptr, "pbr_fxaa_batch: null pointer");
    PBR_REQUIRE(ctx, n >= 1 && n <= (uint32_t)PBR_MAX_VIEWS, "pbr_fxaa_batch: n is not 1 .. PBR_MAX_VIEWS");
    PBR_CHECK(ctx, "pbr_fxaa_batch", fxaa_refusal(images, n, w, h));
    FxaaArgs<true> A;
    A.w = w;
    A.h = h;
    for (uint32_t i = 0; i < (uint32_t)PBR_MAX_VIEWS; i++) A.img[i] = images[i < n ? i : n - 1];
    launch_fxaa<true>(ctx, A, n);
    return pbr::launched(ctx, "k_fxaa");
}

}  // extern "C"
