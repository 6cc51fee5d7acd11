// gbuffer_raster.hip — GBufferPass::Execute + DrawModel (DeferredPipeline.cpp:138-185): gbuffer.hlsl's vertex shader (:71-86), the
// fixed-function stages of DefaultOpaque (back faces culled, FrontCounterClockwise = FALSE; depth LESS with write; stencil ALWAYS,
// INCR_SAT on depth pass) and ps_main (:88-149), as a sort-middle pipeline in the style of Laine & Karras ("High-Performance Software
// Rasterization on GPUs", HPG 2011) on the caller's scratch; and the depth-only raster, which writes that pipeline's depth plane alone.
//
// The rules.  Coverage: exact 64-bit integer edge functions on 16.8 fixed-point vertices at pixel centres, top-left rule.  Depth: z / w
// of the snapped vertices interpolated linearly in screen space (fp64, rounded once to fp32), clamped to [0, 1].  Normals: the
// triangle's perspective-correct barycentrics from its 2D homogeneous edge planes (Olano & Greer 1997), so a clipped polygon resolves
// against the triangle it came from; the planes are formed in fp64 about an integer pixel origin near the triangle (the centre of its
// snapped polygon's bounding box within the frame) and rounded once to fp32, and the resolve evaluates them at the pixel's exact offset
// from that origin, so their accuracy does not depend on where in the frame the triangle lies.  Built with -ffp-contract=off:
// tests/raster_ref.py (raster_tex_ref.py, raster_cull_ref.py) restates every step in the same operation order; tests/raster_truth.py,
// raster_cover_truth.py and sampler_truth.py hold the results to fp64 statements of the contract.
//
// The file, in order; every piece that two kernels or two entry points use is stated once:
//   records and layout   RsTri (the clipped, snapped polygon), RsAttr / RsTexAttr (the resolve's records), the scratch Layout, RsParams,
//                        the argument packs that select a kernel variant (empty pack = the constant-material / unculled kernel)
//   k_rs_clear           zero the per-bin counters
//   k_rs_prep            one block: the first triangle of every draw (exclusive scan of index_count / 3) and the triangle count.  Pack
//                        RsCull = the model cull (pbr_raster_desc.bounds; Scene::CullModel on the device): a draw whose world box lies
//                        outside one of the six planes of the widened tile (pinned in pbr_hip.h; formed on the host in fp64 per call by
//                        cull_planes) gets no triangles in the scan, so no later kernel sees it.  k_rs_bounds (pbr_draw_bounds) makes
//                        the draws' local boxes.
//   walk_bins<COOP>      the bin walk of setup (counts) and fill (appends): per lane, or, depth chain, a box of more than COOP_BINS bins
//                        by the whole wave
//   k_rs_setup           lane = triangle: vertex stage, near / guard-band clip, viewport, 16.8 snap, cull, bounding box, bin counts; the
//                        resolve's planes.  Pack RsSetupTex: also the uv / tangent record, and draws with a bad map index dropped;
//                        pack RsSetupDepth: the raster record and the bin counts only
//   k_rs_scan            one wave: every bin's list offset in the pool, in raster order; a list that does not fit, or is longer than
//                        LIST_CAP, takes none.  k_rs_scan_depth: a block-wide prefix sum; a list is refused for lack of space only
//   k_rs_fill[_depth]    lane = triangle: its id into the list of every bin its box touches (append_id, in any order), by either walk
//   the bin kernels' shared pieces   RS_BIN_PIXEL, RS_FOR_EACH_FRAGMENT (the coverage and depth rule of BOTH chains: pbr_depth_raster's
//                        bit-exactness contract rests on it), every_record (a bin without a list walks every triangle record in draw
//                        order and tests its box: the same triangles in the same order, so the same bits, only slower), RsWeights
//   k_rs_raster          block = 16 x 16-pixel bin, lane = pixel: the bin's list sorted in LDS (draw order), depth, stencil and the
//                        winning triangle in registers, then the winner's attributes and the G-buffer encode (gbuffer_encode.hpp).
//                        Packs RsRasterTex / RsRasterTexBc1 (pbr_raster_desc.maps; a table that holds a PBR_TEX_BC1_BLOCKS texture): the
//                        perspective-correct uv / tangent, the quad's LOD, up to five trilinear samples (tex_sampler.hpp; BC1 taps from
//                        the blocks in place, bc1_decode.hpp) and the normal-map frame before the same encode
//   k_rs_depth           block = bin, lane = pixel: min(1, min over the covering fragments of z), a minimum over a totally ordered set
//                        (z is clamped, a NaN is 0, -0 never occurs), so the list is walked unsorted from the pool, whatever its
//                        length, DEPTH_CHUNK raster records at a time staged in LDS
//   the host side        RsCall (the fields both descriptors have), cull_refusal / call_refusal (the shared checks; each entry point
//                        refuses under its own name), params, Carve (the scratch by its layout), launch_clear_prep; raster() and
//                        depth_raster(): their own checks and their six launches; the exports
#include "pbr_internal.hpp"
#include "pbr_device.hpp"
#include "tex_chain.hpp"
#include <cfloat>
#include <type_traits>

using namespace pbr;

namespace {

#include "gbuffer_encode.hpp"
#include "texel_decode.hpp"
#include "bc1_decode.hpp"
using tex2d::bc1_blocks;
#include "tex_sampler.hpp"

constexpr uint32_t BIN = 16;               // bin edge in pixels: 256 lanes, one per pixel
constexpr uint32_t LIST_CAP = 2048;        // longest bin list sorted in LDS
constexpr uint32_t DEPTH_CHUNK = 128;      // depth chain: raster records staged in LDS per round of a bin's list
constexpr uint32_t COOP_BINS = 64;         // depth chain: a box of more bins than this is binned by its whole wave
constexpr float GUARD = 128.0f;            // guard band: |x|, |y| <= GUARD * w (clip space) needs no x / y clipping
constexpr uint32_t MAX_POLY = 8;           // a triangle clipped by five planes
constexpr uint32_t NONE = 0xffffffffu;

// raster record: the clipped, snapped polygon (a fan from vertex 0) in global 16.8 fixed point
struct alignas(16) RsTri {
    uint32_t n;                            // vertices; 0 = nothing to rasterize
    uint32_t lo, hi;                       // pixel bounding box clamped to the tile, global pixels x | y << 16, inclusive
    uint32_t pad;
    int32_t X[MAX_POLY], Y[MAX_POLY];
    float Z[MAX_POLY];
};
static_assert(sizeof(RsTri) == 112, "raster record layout");
// resolve record: lambda_i(px, py) = (c[3i] * (px - ox) + c[3i+1] * (py - oy)) + c[3i+2] (screen pixels; the origin is a function
// of the triangle and the frame, never of the tile), normal_ws of vertex i = n[3i..3i+2]
struct RsAttr {
    float c[9];
    float n[9];
    uint32_t draw;
    uint32_t origin;                       // ox | oy << 16, each in [0, PBR_RASTER_MAX_SIZE]
};
static_assert(sizeof(RsAttr) == 80, "resolve record layout");
// textured resolve record: uv of vertex i = uv[2i..2i+1], tangent_ws of vertex i = t[3i..3i+2]
struct RsTexAttr {
    float uv[6];
    float t[9];
    uint32_t pad;
};
static_assert(sizeof(RsTexAttr) == 64, "textured resolve record layout");

// scratch layout (byte offsets, 256-aligned); everything up to `pool` is the minimum.  The textured layout adds `tex`; the depth-only
// layout (resolve = false) has no `attrs`.
struct Layout {
    size_t draw_base, count, cursor, offset, tris, attrs, tex, pool;
    uint32_t nbx, nby;
};
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline Layout layout(uint32_t w, uint32_t h, uint32_t n_triangles, bool textured = false, bool resolve = true) {
    Layout L;
    L.nbx = (w + BIN - 1) / BIN;
    L.nby = (h + BIN - 1) / BIN;
    const size_t bins = (size_t)L.nbx * L.nby;
    L.draw_base = 256;                                           // [0, 256): header, word 0 = triangle count
    L.count = L.draw_base + align256(((size_t)PBR_RASTER_MAX_DRAWS + 1) * 4);
    L.cursor = L.count + align256(bins * 4);
    L.offset = L.cursor + align256(bins * 4);
    L.tris = L.offset + align256(bins * 4);
    L.attrs = L.tris + align256((size_t)n_triangles * sizeof(RsTri));
    L.tex = L.attrs + (resolve ? align256((size_t)n_triangles * sizeof(RsAttr)) : 0);
    L.pool = L.tex + (textured ? align256((size_t)n_triangles * sizeof(RsTexAttr)) : 0);
    return L;
}

struct RsParams {
    float View[16], Projection[16];
    float half_w, half_h;
    uint32_t full_w, full_h;
    uint32_t x0, y0, w, h;
    uint32_t nbx;
    uint32_t n_vertices, n_indices, n_draws;
    uint32_t pitch;
    uint32_t pool_cap;                     // entries of the list pool
};

// the textured kernels' extra arguments
struct RsSetupTex {
    const pbr_draw_maps* maps;
    RsTexAttr* tex;
    uint32_t n_tex;
};
struct RsRasterTex {
    const pbr_draw_maps* maps;
    const RsTexAttr* tex;
    uint32_t n_tex;
    pbr_texture2d table[PBR_RASTER_MAX_TEXTURES];
};
// the same arguments for a table that holds a BC1-resident texture (PBR_TEX_BC1_BLOCKS): a kernel of its own, picked on the host,
// so a table of decoded textures keeps the kernel it had
struct RsRasterTexBc1 : RsRasterTex {};
// k_rs_setup's pack in the depth-only chain: no resolve record at all (attrs is null)
struct RsSetupDepth {};
// k_rs_prep's extra argument in the culled calls
struct RsCull {
    const pbr_aabb* bounds;
    pbr_cull_stats* stats;                 // may be null
    float planes[24];                      // left, right, bottom, top, near, far: inside <=> dot(p, (x, 1)) >= 0
};
// the one element of a non-empty `Tex` / `Cull` pack
template <typename T> __device__ __forceinline__ const T& only(const T& t) { return t; }

struct ClipV { float x, y, z, w; };

// row r of a row-major matrix times (x, y, z, w): mul(M, v), summed left to right
__device__ __forceinline__ float row4(const float* m, float x, float y, float z, float w) {
    return ((m[0] * x + m[1] * y) + m[2] * z) + m[3] * w;
}
// component i of transpose(InvModel) (v, 0), summed left to right: gbuffer.hlsl's rule for a normal and for a tangent
__device__ __forceinline__ float inv_transpose3(const float* im, int i, const float* v) {
    return ((im[i] * v[0] + im[4 + i] * v[1]) + im[8 + i] * v[2]) + im[12 + i] * 0.0f;
}
// clip planes: 0 near (z >= 0), 1-4 the guard band (x >= -G w, x <= G w, y >= -G w, y <= G w); inside <=> d >= 0
__device__ __forceinline__ float plane_d(const ClipV& v, uint32_t pl) {
    switch (pl) {
        case 0: return v.z;
        case 1: return v.x + GUARD * v.w;
        case 2: return GUARD * v.w - v.x;
        case 3: return v.y + GUARD * v.w;
        default: return GUARD * v.w - v.y;
    }
}

// exclusive scan over a block of 1024 lanes; `total` = the block's sum
__device__ uint64_t block_scan_1024(uint64_t v, uint64_t* lds, uint64_t& total) {
    const uint32_t t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (uint32_t off = 1; off < 1024u; off <<= 1) {
        const uint64_t a = t >= off ? lds[t - off] : 0;
        __syncthreads();
        lds[t] += a;
        __syncthreads();
    }
    total = lds[1023];
    const uint64_t incl = lds[t];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(256) void k_rs_clear(uint32_t* __restrict__ count, uint32_t* __restrict__ cursor, uint32_t n) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        count[i] = 0;
        cursor[i] = 0;
    }
}

// the model cull of pbr_hip.h, operation for operation: true = the draw's world box lies outside one of the six planes by more than
// the slack.  Every comparison is written so that a NaN keeps the draw.
__device__ __forceinline__ bool draw_culled(const pbr_draw& d, const pbr_aabb& b, const float* __restrict__ planes) {
    const float* M = d.Model;
    bool can = M[12] == 0.0f && M[13] == 0.0f && M[14] == 0.0f && M[15] == 1.0f;
    float c[3], e[3], cw[3], ew[3];
    for (int i = 0; i < 3; i++) {
        can = can && b.min[i] <= b.max[i] && fabsf(b.min[i]) <= FLT_MAX && fabsf(b.max[i]) <= FLT_MAX;
        c[i] = (b.min[i] + b.max[i]) * 0.5f;
        e[i] = (b.max[i] - b.min[i]) * 0.5f;
    }
    for (int i = 0; i < 3; i++) {
        cw[i] = ((M[4 * i] * c[0] + M[4 * i + 1] * c[1]) + M[4 * i + 2] * c[2]) + M[4 * i + 3];
        ew[i] = (fabsf(M[4 * i]) * e[0] + fabsf(M[4 * i + 1]) * e[1]) + fabsf(M[4 * i + 2]) * e[2];
    }
    bool out = false;
    for (int k = 0; k < 6; k++) {
        const float* p = planes + 4 * k;
        const float dist = ((p[0] * cw[0] + p[1] * cw[1]) + p[2] * cw[2]) + p[3];
        const float h = (fabsf(p[0] * ew[0]) + fabsf(p[1] * ew[1])) + fabsf(p[2] * ew[2]);
        const float S = (((fabsf(p[0] * cw[0]) + fabsf(p[1] * cw[1])) + fabsf(p[2] * cw[2])) + fabsf(p[3])) + h;
        out = out || dist < -(h + 0x1p-16f * S);
    }
    return can && out;
}

// draw_base[d] = first triangle id of draw d (index_count / 3 triangles each, in draw order), clamped to max_tris;
// hdr[0] = the number of triangles rasterized (ids >= max_tris are not)
// Cull: empty, or RsCull (a culled draw has no triangles; thread 0 writes the call's pbr_cull_stats).  The culled variant parks each
// draw's count in draw_base[d] between the test and the two passes of the scan, so the test runs once per draw; the scan itself is
// one text, with the per-draw count (`count`) as the only difference.
template <typename... Cull>
__global__ __launch_bounds__(1024) void k_rs_prep(const pbr_draw* __restrict__ draws, uint32_t n_draws, uint32_t max_tris,
                                                  uint32_t* __restrict__ draw_base, uint32_t* __restrict__ hdr, Cull... cull) {
    constexpr bool CULL = sizeof...(Cull) != 0;
    __shared__ uint64_t lds[1024];
    __shared__ unsigned long long gone[2];           // culled draws, culled triangles (CULL only)
    const uint32_t per = (n_draws + 1023u) / 1024u;
    const uint32_t b = min(threadIdx.x * per, n_draws), e = min(b + per, n_draws);
    uint32_t nd = 0;
    uint64_t nt = 0;
    if constexpr (CULL) {
        const RsCull& cl = only(cull...);
        if (threadIdx.x == 0) { gone[0] = 0; gone[1] = 0; }
        // the test, draw = k * 1024 + thread: neighbouring lanes read neighbouring records and share their cache lines (a thread's own
        // range [b, e) puts the lanes of one load `per` records apart)
        for (uint32_t d = threadIdx.x; d < n_draws; d += 1024u) {
            uint32_t n = draws[d].index_count / 3u;
            if (draw_culled(draws[d], cl.bounds[d], cl.planes)) {
                nd++;
                nt += n;
                n = 0;
            }
            draw_base[d] = n;
        }
        __syncthreads();                                   // the parked counts are read by other threads of the block
    }
    const auto count = [&](uint32_t d) -> uint32_t {
        if constexpr (CULL) return draw_base[d]; else return draws[d].index_count / 3u;
    };
    uint64_t s = 0;
    for (uint32_t d = b; d < e; d++) s += count(d);
    uint64_t total;
    uint64_t run = block_scan_1024(s, lds, total);
    if constexpr (CULL)
        if (nd) {
            atomicAdd(&gone[0], (unsigned long long)nd);
            atomicAdd(&gone[1], (unsigned long long)nt);
        }
    for (uint32_t d = b; d < e; d++) {
        const uint32_t n = count(d);
        draw_base[d] = (uint32_t)min(run, (uint64_t)max_tris);
        run += n;
    }
    if constexpr (CULL) __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t n = (uint32_t)min(total, (uint64_t)max_tris);
        draw_base[n_draws] = n;
        hdr[0] = n;
        if constexpr (CULL) {
            const RsCull& cl = only(cull...);
            if (cl.stats) {
                pbr_cull_stats st;
                st.draws_culled = (uint32_t)gone[0];
                st.draws_drawn = n_draws - st.draws_culled;
                st.triangles_drawn = n;
                st.triangles_culled = (uint32_t)min(gone[1], 0xffffffffull);
                *cl.stats = st;
            }
        }
    }
}

// pbr_draw_bounds: block = draw, lane = triangle (strided).  min / max run on an order-preserving integer key of the float
// (-0 below +0; a NaN position takes no part), so the result does not depend on the order of the reduction.
__device__ __forceinline__ uint32_t bound_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float bound_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__global__ __launch_bounds__(256) void k_rs_bounds(const pbr_vertex* __restrict__ vtx, uint32_t n_vertices, const uint32_t* __restrict__ idx,
                                                   uint32_t n_indices, const pbr_draw* __restrict__ draws, pbr_aabb* __restrict__ out) {
    __shared__ uint32_t part[4][6];
    const pbr_draw& d = draws[blockIdx.x];
    const uint32_t first = d.first_index, count = d.index_count;
    const int64_t base = d.base_vertex;
    uint32_t lo[3], hi[3];
    for (int i = 0; i < 3; i++) { lo[i] = bound_key(FLT_MAX); hi[i] = bound_key(-FLT_MAX); }
    // the guards of k_rs_setup: a range past n_indices is skipped whole, a triangle with an index outside the vertex buffer is dropped
    if ((uint64_t)first + count <= n_indices) {
        for (uint32_t t = threadIdx.x; t < count / 3u; t += 256u) {
            int64_t vi[3];
            bool ok = true;
            for (int k = 0; k < 3; k++) {
                vi[k] = (int64_t)idx[(uint64_t)first + 3ull * t + k] + base;
                ok = ok && vi[k] >= 0 && vi[k] < (int64_t)n_vertices;
            }
            if (!ok) continue;
            for (int k = 0; k < 3; k++)
                for (int i = 0; i < 3; i++) {
                    const float v = vtx[vi[k]].position[i];
                    if (v == v) {
                        lo[i] = min(lo[i], bound_key(v));
                        hi[i] = max(hi[i], bound_key(v));
                    }
                }
        }
    }
    for (int i = 0; i < 3; i++)
        for (uint32_t off = 32; off > 0; off >>= 1) {
            lo[i] = min(lo[i], (uint32_t)__shfl_down((int)lo[i], off));
            hi[i] = max(hi[i], (uint32_t)__shfl_down((int)hi[i], off));
        }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0)
        for (int i = 0; i < 3; i++) { part[wave][i] = lo[i]; part[wave][3 + i] = hi[i]; }
    __syncthreads();
    if (threadIdx.x == 0) {
        pbr_aabb r;
        for (int i = 0; i < 3; i++) {
            r.min[i] = bound_unkey(min(min(part[0][i], part[1][i]), min(part[2][i], part[3][i])));
            r.max[i] = bound_unkey(max(max(part[0][3 + i], part[1][3 + i]), max(part[2][3 + i], part[3][3 + i])));
        }
        out[blockIdx.x] = r;
    }
}

// The bin walk of k_rs_setup (f counts) and of the fill kernels (f appends): f(bin, id) for every bin of the lane's box
// [bx0, bx1] x [by0, by1] (`has`: the lane has one).  Two forms, one call shape:
//   COOP = false (the G-buffer chain): each lane walks its own box;
//   COOP = true (the depth chain): a box of at most COOP_BINS bins is walked by its lane; a larger one by the 64 lanes of the wave, one
//   such box after the other, so a triangle that fills a 2048^2 map costs 256 rounds of 64 atomics, not 16 384 atomics of one lane.
//   Every lane of the wave that has not left the kernel calls this at the same point; the lanes that have (triangle ids past the
//   count) take no part, so the walk strides by the number of lanes that are here, each at its rank among them.
template <bool COOP, typename F>
__device__ __forceinline__ void walk_bins(bool has, uint32_t bx0, uint32_t by0, uint32_t bx1, uint32_t by1, uint32_t nbx, uint32_t id, F f) {
    const bool big = COOP && has && (bx1 - bx0 + 1u) * (by1 - by0 + 1u) > COOP_BINS;
    if (has && !big)
        for (uint32_t by = by0; by <= by1; by++)
            for (uint32_t bx = bx0; bx <= bx1; bx++) f(by * nbx + bx, id);
    if constexpr (COOP) {
        const unsigned long long here = __ballot(1);
        const uint32_t lanes = (uint32_t)__popcll(here), rank = (uint32_t)__popcll(here & ((1ull << (threadIdx.x & 63u)) - 1ull));
        for (unsigned long long m = __ballot(big); m; m &= m - 1ull) {
            const int src = __ffsll(m) - 1;
            const uint32_t x0 = __shfl(bx0, src), y0 = __shfl(by0, src), x1 = __shfl(bx1, src), y1 = __shfl(by1, src), sid = __shfl(id, src);
            const uint32_t nx = x1 - x0 + 1u, total = nx * (y1 - y0 + 1u);
            for (uint32_t i = rank; i < total; i += lanes) f((y0 + i / nx) * nbx + (x0 + i % nx), sid);
        }
    }
}

// Tex: empty (constant materials), RsSetupTex (textured: the uv / tangent record, and the map-index guard) or RsSetupDepth (the
// depth-only chain: the raster record and the bin counts only)
template <typename... Tex>
__global__ __launch_bounds__(256) void k_rs_setup(RsParams p, const pbr_vertex* __restrict__ vtx, const uint32_t* __restrict__ idx,
                                                  const pbr_draw* __restrict__ draws, const uint32_t* __restrict__ draw_base,
                                                  const uint32_t* __restrict__ hdr, RsTri* __restrict__ tris,
                                                  RsAttr* __restrict__ attrs, uint32_t* __restrict__ bin_count, Tex... tex) {
    constexpr bool DEPTH = (std::is_same<Tex, RsSetupDepth>::value || ...);
    constexpr bool TEX = sizeof...(Tex) != 0 && !DEPTH;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= hdr[0]) return;
    uint32_t lo = 0, hi = p.n_draws - 1;        // the draw: the last d with draw_base[d] <= t
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (draw_base[mid] <= t) lo = mid; else hi = mid - 1u;
    }
    const pbr_draw& d = draws[lo];
    RsTri rec;
    rec.n = 0; rec.lo = 0; rec.hi = 0; rec.pad = 0;
    // the resolve record is stored in two halves: the normals and the draw after the vertex stage, the planes and their origin once
    // the polygon is snapped (zero for a triangle that draws nothing), so the two are not live at once
    float an[9], ac[9];
    for (int i = 0; i < 9; i++) { an[i] = 0.0f; ac[i] = 0.0f; }
    uint32_t origin = 0;
    // the bin counts: the box in bins (`binned`: the triangle has one) and what walk_bins does with each bin of it
    bool binned = false;
    uint32_t bx0 = 0, by0 = 0, bx1 = 0, by1 = 0;
    const auto count_bin = [&](uint32_t b, uint32_t) { atomicAdd(&bin_count[b], 1u); };
    // guard (device data): a draw range past n_indices, or an index (+ base_vertex) outside [0, n_vertices): the triangle is dropped
    const uint64_t first = (uint64_t)d.first_index + 3ull * (t - draw_base[lo]);
    bool ok = (uint64_t)d.first_index + d.index_count <= p.n_indices;
    if constexpr (TEX) {
        // and a draw with a map index past the texture table
        const RsSetupTex& tx = only(tex...);
        const pbr_draw_maps m = tx.maps[lo];
        for (const uint32_t k : {m.albedo, m.normal, m.roughness, m.metallic, m.ao}) ok = ok && (k == PBR_NO_MAP || k < tx.n_tex);
    }
    int64_t vi[3] = {0, 0, 0};
    for (int k = 0; k < 3 && ok; k++) {
        vi[k] = (int64_t)idx[first + k] + d.base_vertex;
        ok = vi[k] >= 0 && vi[k] < (int64_t)p.n_vertices;
    }
    ClipV c[3];
    if (ok) {
        for (int k = 0; k < 3; k++) {
            const pbr_vertex& v = vtx[vi[k]];
            // gbuffer.hlsl:77-82: position_ws = Model (p, 1); normal_ws = transpose(InvModel) (n, 0); clip = Projection (View position_ws)
            float pw[4], pv[4];
            for (int r = 0; r < 4; r++) pw[r] = row4(d.Model + 4 * r, v.position[0], v.position[1], v.position[2], 1.0f);
            for (int r = 0; r < 4; r++) pv[r] = row4(p.View + 4 * r, pw[0], pw[1], pw[2], pw[3]);
            c[k].x = row4(p.Projection + 0, pv[0], pv[1], pv[2], pv[3]);
            c[k].y = row4(p.Projection + 4, pv[0], pv[1], pv[2], pv[3]);
            c[k].z = row4(p.Projection + 8, pv[0], pv[1], pv[2], pv[3]);
            c[k].w = row4(p.Projection + 12, pv[0], pv[1], pv[2], pv[3]);
            if constexpr (!DEPTH)
                for (int i = 0; i < 3; i++) an[3 * k + i] = inv_transpose3(d.InvModel, i, v.normal);
        }
    }
    if constexpr (!DEPTH) {
        for (int i = 0; i < 9; i++) attrs[t].n[i] = an[i];
        attrs[t].draw = lo;
    }
    if constexpr (TEX) {
        // gbuffer.hlsl:80-84: tangent_ws = transpose(InvModel) (t, 0) (the normal's rule), uv as given; computed after the resolve
        // record is stored, so the two records are not live at once
        RsTexAttr ta;
        for (int i = 0; i < 6; i++) ta.uv[i] = 0.0f;
        for (int i = 0; i < 9; i++) ta.t[i] = 0.0f;
        ta.pad = 0;
        if (ok) {
            for (int k = 0; k < 3; k++) {
                const pbr_vertex& v = vtx[vi[k]];
                for (int i = 0; i < 3; i++) ta.t[3 * k + i] = inv_transpose3(d.InvModel, i, v.tangent);
                ta.uv[2 * k] = v.uv[0];
                ta.uv[2 * k + 1] = v.uv[1];
            }
        }
        only(tex...).tex[t] = ta;
    }
    if (ok) {
        // clip against the near plane and, outside the guard band, its four planes (Sutherland-Hodgman; a plane no vertex is
        // outside of is skipped).  A new vertex is computed from its edge's inside endpoint towards the outside one, so two
        // triangles that share the edge get the same point.
        ClipV poly[MAX_POLY], tmp[MAX_POLY];
        uint32_t n = 3;
        poly[0] = c[0]; poly[1] = c[1]; poly[2] = c[2];
        for (uint32_t pl = 0; pl < 5 && n >= 3; pl++) {
            bool any_out = false;
            for (uint32_t i = 0; i < n; i++) any_out |= !(plane_d(poly[i], pl) >= 0.0f);
            if (!any_out) continue;
            // in exact arithmetic a plane adds at most one vertex (3 + 5 = MAX_POLY); rounding near a plane can make more sign
            // changes: such a polygon is dropped (m counts on, nothing is written past MAX_POLY)
            uint32_t m = 0;
            for (uint32_t i = 0; i < n; i++) {
                const ClipV a = poly[i], b = poly[i + 1 == n ? 0 : i + 1];
                const float da = plane_d(a, pl), db = plane_d(b, pl);
                const bool ia = da >= 0.0f, ib = db >= 0.0f;
                if (ia) {
                    if (m < MAX_POLY) tmp[m] = a;
                    m++;
                }
                if (ia != ib) {
                    const ClipV in = ia ? a : b, out = ia ? b : a;
                    const float din = ia ? da : db, dout = ia ? db : da;
                    const float s = din / (din - dout);
                    if (m < MAX_POLY)
                        tmp[m] = ClipV{in.x + (out.x - in.x) * s, in.y + (out.y - in.y) * s, in.z + (out.z - in.z) * s,
                                       in.w + (out.w - in.w) * s};
                    m++;
                }
            }
            n = m <= MAX_POLY ? m : 0;
            for (uint32_t i = 0; i < n; i++) poly[i] = tmp[i];
        }
        // viewport (0, 0, full_w, full_h), snap to 1/256 pixel (round to nearest even), depth z / w
        bool good = n >= 3;
        for (uint32_t i = 0; i < n && good; i++) {
            const float xn = poly[i].x / poly[i].w, yn = poly[i].y / poly[i].w;
            good = poly[i].w > 0.0f && fabsf(xn) <= 2.0f * GUARD && fabsf(yn) <= 2.0f * GUARD;
            if (good) {
                rec.X[i] = (int32_t)rintf(((xn + 1.0f) * p.half_w) * 256.0f);
                rec.Y[i] = (int32_t)rintf(((1.0f - yn) * p.half_h) * 256.0f);
                rec.Z[i] = poly[i].z / poly[i].w;
            }
        }
        // something to draw: a front-facing (clockwise in y-down screen space) fan triangle of non-zero area
        bool front = false;
        for (uint32_t k = 1; good && k + 1 < n; k++) {
            const int64_t area = (int64_t)(rec.X[k] - rec.X[0]) * (rec.Y[k + 1] - rec.Y[0]) -
                                 (int64_t)(rec.Y[k] - rec.Y[0]) * (rec.X[k + 1] - rec.X[0]);
            front |= area > 0;
        }
        if (good && front) {
            int32_t x0 = rec.X[0], x1 = rec.X[0], y0 = rec.Y[0], y1 = rec.Y[0];
            for (uint32_t i = 1; i < n; i++) {
                x0 = min(x0, rec.X[i]); x1 = max(x1, rec.X[i]);
                y0 = min(y0, rec.Y[i]); y1 = max(y1, rec.Y[i]);
            }
            if constexpr (!DEPTH) {
                // the resolve's origin: the centre of the polygon's bounding box within the frame, floored to a pixel
                const int32_t fw8 = (int32_t)(p.full_w << 8), fh8 = (int32_t)(p.full_h << 8);
                const int32_t ox = (min(max(x0, 0), fw8) + min(max(x1, 0), fw8)) >> 9, oy = (min(max(y0, 0), fh8) + min(max(y1, 0), fh8)) >> 9;
                // the triangle's 2D homogeneous screen vertices (sx / w, sy / w = the viewport transform) about that origin and their
                // edge planes, in fp64 (the translation cancels what the products would otherwise have to), each rounded once
                double sx[3], sy[3], sw[3];
                for (int k = 0; k < 3; k++) {
                    sw[k] = (double)c[k].w;
                    sx[k] = ((double)c[k].x + sw[k]) * (double)p.half_w - (double)ox * sw[k];
                    sy[k] = (sw[k] - (double)c[k].y) * (double)p.half_h - (double)oy * sw[k];
                }
                for (int i = 0; i < 3; i++) {
                    const int j = (i + 1) % 3, k = (i + 2) % 3;
                    ac[3 * i + 0] = (float)(sy[j] * sw[k] - sw[j] * sy[k]);
                    ac[3 * i + 1] = (float)(sw[j] * sx[k] - sx[j] * sw[k]);
                    ac[3 * i + 2] = (float)(sx[j] * sy[k] - sy[j] * sx[k]);
                }
                origin = (uint32_t)ox | ((uint32_t)oy << 16);
            }
            // pixels whose centre (256 x + 128) lies in [x0, x1], clamped to the tile
            const int64_t px0 = max(-((128 - (int64_t)x0) >> 8), (int64_t)p.x0), px1 = min(((int64_t)x1 - 128) >> 8, (int64_t)(p.x0 + p.w) - 1);
            const int64_t py0 = max(-((128 - (int64_t)y0) >> 8), (int64_t)p.y0), py1 = min(((int64_t)y1 - 128) >> 8, (int64_t)(p.y0 + p.h) - 1);
            if (px0 <= px1 && py0 <= py1) {
                rec.n = n;
                rec.lo = (uint32_t)px0 | ((uint32_t)py0 << 16);
                rec.hi = (uint32_t)px1 | ((uint32_t)py1 << 16);
                binned = true;
                bx0 = ((uint32_t)px0 - p.x0) / BIN; bx1 = ((uint32_t)px1 - p.x0) / BIN;
                by0 = ((uint32_t)py0 - p.y0) / BIN; by1 = ((uint32_t)py1 - p.y0) / BIN;
                // each lane on its own: here.  (One call site for both forms, after the lanes have come together, costs these two
                // instantiations vector instructions and waits; the walk itself is stated once.)
                if constexpr (!DEPTH) walk_bins<false>(true, bx0, by0, bx1, by1, p.nbx, t, count_bin);
            }
        }
    }
    if constexpr (DEPTH) {
        walk_bins<true>(binned, bx0, by0, bx1, by1, p.nbx, t, count_bin);      // by the wave: once the lanes have come together again
    } else {
        for (int i = 0; i < 9; i++) attrs[t].c[i] = ac[i];
        attrs[t].origin = origin;
    }
    tris[t] = rec;
}

// offset[b] = start of bin b's list in the pool, or NONE: bins in raster order take the pool's next entries while their list
// fits; a list that does not fit, or is longer than LIST_CAP, gets NONE and takes nothing (a later, shorter list may still fit).
// One wave: a shuffle scan of 64 counts at a time, restarted behind each list that is refused.
__global__ __launch_bounds__(64) void k_rs_scan(const uint32_t* __restrict__ count, uint32_t n_bins, uint32_t pool_cap,
                                                uint32_t* __restrict__ offset) {
    const uint32_t lane = threadIdx.x;
    unsigned long long run = 0;
    for (uint32_t base = 0; base < n_bins;) {
        const uint32_t i = base + lane;
        const unsigned long long c = i < n_bins ? count[i] : 0ull;
        unsigned long long inc = c;
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            const unsigned long long y = __shfl_up(inc, off);
            if (lane >= off) inc += y;
        }
        const bool refused = c != 0 && (c > LIST_CAP || run + inc > pool_cap);
        const unsigned long long mask = __ballot(refused);
        const uint32_t stop = mask ? (uint32_t)__ffsll(mask) - 1u : 64u;   // lanes below `stop` fit
        if (i < n_bins && lane < stop) offset[i] = (uint32_t)(run + inc - c);
        if (i < n_bins && lane == stop) offset[i] = NONE;
        if (stop > 0) run += __shfl(inc, (int)stop - 1);
        base += stop < 64u ? stop + 1u : 64u;
    }
}

// what the fill kernels do with each bin of a triangle's box: the triangle's id into the bin's list, if the bin has one
__device__ __forceinline__ void append_id(const uint32_t* __restrict__ offset, uint32_t* __restrict__ cursor, uint32_t* __restrict__ pool,
                                          uint32_t b, uint32_t id) {
    const uint32_t off = offset[b];
    if (off != NONE) pool[off + atomicAdd(&cursor[b], 1u)] = id;
}

// lane = triangle: its id into the list of every bin its box touches (in any order: k_rs_raster sorts).  k_rs_fill_depth is this
// kernel with the other form of the walk; as one body with two instantiations this one's entry code moved (profiles/raster_isa_resources.md)
__global__ __launch_bounds__(256) void k_rs_fill(RsParams p, const uint32_t* __restrict__ hdr, const RsTri* __restrict__ tris,
                                                 const uint32_t* __restrict__ offset, uint32_t* __restrict__ cursor,
                                                 uint32_t* __restrict__ pool) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= hdr[0]) return;
    const RsTri& r = tris[t];
    if (r.n == 0) return;
    const uint32_t px0 = (r.lo & 0xffffu) - p.x0, py0 = (r.lo >> 16) - p.y0, px1 = (r.hi & 0xffffu) - p.x0, py1 = (r.hi >> 16) - p.y0;
    walk_bins<false>(true, px0 / BIN, py0 / BIN, px1 / BIN, py1 / BIN, p.nbx, t,
                     [&](uint32_t b, uint32_t id) { append_id(offset, cursor, pool, b, id); });
}

// the depth chain's k_rs_scan: a minimum does not need its list sorted in LDS, so no list is too long, and which bins go without
// a list changes no bit, so the scan is a plain prefix sum by one block: bins in raster order take the pool's next entries until a
// list would end past the pool; that bin and the bins after it get NONE
__global__ __launch_bounds__(1024) void k_rs_scan_depth(const uint32_t* __restrict__ count, uint32_t n_bins, uint32_t pool_cap,
                                                        uint32_t* __restrict__ offset) {
    __shared__ uint64_t lds[1024];
    const uint32_t per = (n_bins + 1023u) / 1024u;
    const uint32_t b = min(threadIdx.x * per, n_bins), e = min(b + per, n_bins);
    uint64_t s = 0;
    for (uint32_t i = b; i < e; i++) s += count[i];
    uint64_t total;
    uint64_t run = block_scan_1024(s, lds, total);
    for (uint32_t i = b; i < e; i++) {
        const uint32_t c = count[i];
        run += c;
        offset[i] = run <= pool_cap ? (uint32_t)(run - c) : NONE;
    }
}

// the depth chain's k_rs_fill: the same entries (in any order: a minimum does not care), a large box by the whole wave
__global__ __launch_bounds__(256) void k_rs_fill_depth(RsParams p, const uint32_t* __restrict__ hdr, const RsTri* __restrict__ tris,
                                                       const uint32_t* __restrict__ offset, uint32_t* __restrict__ cursor,
                                                       uint32_t* __restrict__ pool) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= hdr[0]) return;
    const RsTri& r = tris[t];
    const uint32_t px0 = (r.lo & 0xffffu) - p.x0, py0 = (r.lo >> 16) - p.y0, px1 = (r.hi & 0xffffu) - p.x0, py1 = (r.hi >> 16) - p.y0;
    walk_bins<true>(r.n != 0, px0 / BIN, py0 / BIN, px1 / BIN, py1 / BIN, p.nbx, t,
                    [&](uint32_t b, uint32_t id) { append_id(offset, cursor, pool, b, id); });
}

// edge a -> b at P: (Xb - Xa)(PY - Ya) - (Yb - Ya)(PX - Xa); > 0 inside a front-facing triangle.  On the edge (0) a pixel centre is
// covered only by a top edge (horizontal, dx > 0) or a left edge (dy < 0): covered <=> E >= bias, bias = 0 there and 1 elsewhere.
__device__ __forceinline__ int64_t edge_fn(int32_t xa, int32_t ya, int32_t xb, int32_t yb, int64_t PX, int64_t PY) {
    return (int64_t)(xb - xa) * (PY - ya) - (int64_t)(yb - ya) * (PX - xa);
}
__device__ __forceinline__ int64_t edge_bias(int32_t xa, int32_t ya, int32_t xb, int32_t yb) {
    const int32_t dx = xb - xa, dy = yb - ya;
    return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1;
}

// ---- what the two bin kernels (k_rs_raster, k_rs_depth: block = bin, lane = pixel) share, each piece stated once ----
// The pixel and the fragment rule are macros that expand to the text the kernels had, not functions: as a struct and a function template
// taking a lambda they cost k_rs_depth a vector instruction and k_rs_raster<> two SGPRs (profiles/raster_isa_resources.md);
// raster.hip's PBR_SKYBOX_PIXEL is a macro for the same reason.  Both leave lx, ly, inside, gx, gy, PX, PY in the kernel's scope.
// the lane's pixel: in the tile (lx, ly; `inside`: the tile is ragged), in the frame (gx, gy), and its centre in 16.8 fixed point
#define RS_BIN_PIXEL(p, tid)                                                                                                \
    const uint32_t lx = blockIdx.x * BIN + ((tid) & (BIN - 1)), ly = blockIdx.y * BIN + (tid) / BIN;                        \
    const bool inside = lx < (p).w && ly < (p).h;                                                                           \
    [[maybe_unused]] const uint32_t gx = (p).x0 + lx, gy = (p).y0 + ly;                                                     \
    const int64_t PX = (int64_t)((p).x0 + lx) * 256 + 128, PY = (int64_t)((p).y0 + ly) * 256 + 128
// THE FRAGMENT RULE, for both chains (pbr_depth_raster's contract is that its depth plane is pbr_gbuffer_raster's bit for bit):
// the statements `...` run, with `z`, for every fragment of raster record r (the same record for every lane of the block) at
// RS_BIN_PIXEL's pixel: every fan triangle of the polygon, front-facing and of non-zero area; the three edge functions with the
// top-left bias; depth interpolated in fp64, rounded once, clamped to [0, 1] (a NaN to 0).
#define RS_FOR_EACH_FRAGMENT(r, z, ...)                                                                                     \
    {                                                                                                                       \
        const uint32_t n = (r).n;                                                                                           \
        const int32_t X0 = (r).X[0], Y0 = (r).Y[0];                                                                         \
        const float Z0 = (r).Z[0];                                                                                          \
        for (uint32_t k = 1; k + 1 < n; k++) {                                                                              \
            const int32_t X1 = (r).X[k], Y1 = (r).Y[k], X2 = (r).X[k + 1], Y2 = (r).Y[k + 1];                               \
            const int64_t area = (int64_t)(X1 - X0) * (Y2 - Y0) - (int64_t)(Y1 - Y0) * (X2 - X0);                           \
            if (area <= 0) continue; /* back-facing or zero area */                                                         \
            const int64_t w0 = edge_fn(X1, Y1, X2, Y2, PX, PY), w1 = edge_fn(X2, Y2, X0, Y0, PX, PY),                       \
                          w2 = edge_fn(X0, Y0, X1, Y1, PX, PY);                                                             \
            if (inside && w0 >= edge_bias(X1, Y1, X2, Y2) && w1 >= edge_bias(X2, Y2, X0, Y0) && w2 >= edge_bias(X0, Y0, X1, Y1)) { \
                const double z0 = (double)Z0;                                                                               \
                const double zd = z0 + ((double)w1 * ((double)(r).Z[k] - z0) + (double)w2 * ((double)(r).Z[k + 1] - z0)) / (double)area; \
                float z = (float)zd;                                                                                        \
                z = z > 0.0f ? (z < 1.0f ? z : 1.0f) : 0.0f;                                                                \
                __VA_ARGS__                                                                                                 \
            }                                                                                                               \
        }                                                                                                                   \
    }
// THE FALLBACK WALK of a bin without a list: every triangle record in draw order, 256 box tests at a time through list[0 .. 255],
// f(t) for each record whose pixel box touches the bin (t is uniform across the block)
template <typename F>
__device__ __forceinline__ void every_record(const RsParams& p, const uint32_t* __restrict__ hdr, const RsTri* __restrict__ tris,
                                             uint32_t* list, uint32_t tid, F f) {
    const uint32_t rx0 = p.x0 + blockIdx.x * BIN, ry0 = p.y0 + blockIdx.y * BIN;
    const uint32_t rx1 = min(rx0 + BIN, p.x0 + p.w) - 1u, ry1 = min(ry0 + BIN, p.y0 + p.h) - 1u;
    const uint32_t total = hdr[0];
    for (uint32_t base = 0; base < total; base += 256u) {
        const uint32_t t = base + tid;
        uint32_t hit = 0;
        if (t < total) {
            const RsTri& r = tris[t];
            hit = r.n != 0 && (r.lo & 0xffffu) <= rx1 && (r.hi & 0xffffu) >= rx0 && (r.lo >> 16) <= ry1 && (r.hi >> 16) >= ry0;
        }
        list[tid] = hit;
        __syncthreads();
        const uint32_t m = min(256u, total - base);
        for (uint32_t j = 0; j < m; j++)
            if (list[j]) f(base + j);
        __syncthreads();
    }
}
// the barycentric planes of a resolve record at offset (x, y) from its origin, and what they interpolate: attribute values a0, a1, a2
// of the three vertices -> ((l0 a0 + l1 a1) + l2 a2) * inv, perspective-correct
struct RsWeights {
    float l0, l1, l2, inv;
    __device__ __forceinline__ float operator()(float a0, float a1, float a2) const { return ((l0 * a0 + l1 * a1) + l2 * a2) * inv; }
};
__device__ __forceinline__ RsWeights weights_at(const float* c, float x, float y) {
    RsWeights w;
    w.l0 = (c[0] * x + c[1] * y) + c[2];
    w.l1 = (c[3] * x + c[4] * y) + c[5];
    w.l2 = (c[6] * x + c[7] * y) + c[8];
    w.inv = 1.0f / ((w.l0 + w.l1) + w.l2);
    return w;
}

// Tex: empty (constant materials), RsRasterTex (textured: the resolve samples the draw's maps) or RsRasterTexBc1 (textured, and
// some of the textures are BC1-resident)
template <typename... Tex>
__global__ __launch_bounds__(256) void k_rs_raster(RsParams p, const pbr_draw* __restrict__ draws, const uint32_t* __restrict__ hdr,
                                                   const RsTri* __restrict__ tris, const RsAttr* __restrict__ attrs,
                                                   const uint32_t* __restrict__ count, const uint32_t* __restrict__ offset,
                                                   const uint32_t* __restrict__ pool, uint32_t* __restrict__ A, uint32_t* __restrict__ B,
                                                   uint32_t* __restrict__ C, float* __restrict__ depth, uint8_t* __restrict__ stencil,
                                                   Tex... tex) {
    constexpr bool TEX = sizeof...(Tex) != 0;
    constexpr bool BC1 = (std::is_same<Tex, RsRasterTexBc1>::value || ...);
    __shared__ uint32_t list[LIST_CAP];
    const uint32_t tid = threadIdx.x;
    RS_BIN_PIXEL(p, tid);
    float zbuf = 1.0f;
    uint32_t sten = 0, win = NONE;

    // one triangle (t is uniform across the block): depth LESS with write, the winner, stencil INCR_SAT on depth pass
    auto fragment = [&](uint32_t t) {
        const RsTri& r = tris[t];
        RS_FOR_EACH_FRAGMENT(r, z,
            if (z < zbuf) {                      // LESS: strictly nearer than every earlier fragment
                zbuf = z;
                win = t;
                sten = sten < 255u ? sten + 1u : 255u;   // INCR_SAT
            })
    };

    if constexpr (TEX) {
        // the texture table (a uniform loop: no per-lane index into the kernel arguments) and the decode tables into LDS
        TexLds& tl = tex_lds();
        const RsRasterTex& tx = only(tex...);
        for (uint32_t i = 0; i < tx.n_tex; i++)
            if (tid == 0) tl.tex[i] = tx.table[i];
        tl.dec[tid] = kUnorm8[tid];
        tl.dec[256u + tid] = kSrgb8[tid];
        __syncthreads();
    }

    const uint32_t b = blockIdx.y * p.nbx + blockIdx.x;
    const uint32_t cnt = count[b], off = offset[b];
    if (cnt != 0) {
        if (off != NONE && cnt <= LIST_CAP) {
            // the bin's list into LDS and sorted (bitonic): draw order
            uint32_t np2 = 1;
            while (np2 < cnt) np2 <<= 1;
            for (uint32_t i = tid; i < np2; i += 256u) list[i] = i < cnt ? pool[off + i] : NONE;
            __syncthreads();
            for (uint32_t k = 2; k <= np2; k <<= 1)
                for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                    for (uint32_t i = tid; i < np2; i += 256u) {
                        const uint32_t l = i ^ j;
                        if (l > i) {
                            const uint32_t a = list[i], c = list[l];
                            if ((a > c) == ((i & k) == 0)) { list[i] = c; list[l] = a; }
                        }
                    }
                    __syncthreads();
                }
            for (uint32_t i = 0; i < cnt; i++) fragment(__builtin_amdgcn_readfirstlane(list[i]));
        } else {
            every_record(p, hdr, tris, list, tid, fragment);
        }
    }
    // resolve: the winner's perspective-correct normal and its draw's constants -> ps_main's outputs
    uint32_t qa = 0, qb = 0, qc = 0;
    if (win != NONE) {
        const RsAttr& at = attrs[win];
        const pbr_draw& d = draws[at.draw];
        // the pixel centre's offset from the triangle's origin: exact
        const int32_t ox = (int32_t)(at.origin & 0xffffu), oy = (int32_t)(at.origin >> 16);
        const float fx = (float)((int32_t)gx - ox) + 0.5f, fy = (float)((int32_t)gy - oy) + 0.5f;
        const RsWeights l = weights_at(at.c, fx, fy);
        // gbuffer.hlsl:99-146, the Use*Map == false branches: AO = 0 (the reference's value without an AO map)
        float4 a = make_float4(d.Albedo[0], d.Albedo[1], d.Albedo[2], d.Emission);
        float4 b = make_float4(l(at.n[0], at.n[3], at.n[6]), l(at.n[1], at.n[4], at.n[7]), l(at.n[2], at.n[5], at.n[8]), d.Roughness);
        float4 c = make_float4(d.Metallic, 0.0f, 0.0f, 0.0f);
        if constexpr (TEX) {
            const RsRasterTex& tx = only(tex...);
            const pbr_draw_maps m = tx.maps[at.draw];
            if ((m.albedo & m.normal & m.roughness & m.metallic & m.ao) != PBR_NO_MAP) {
                // the Use*Map == true branches (gbuffer.hlsl:62-69,99-141)
                const TexLds& tl = tex_lds();
                const RsTexAttr& ta = tx.tex[win];
                // perspective-correct uv at an offset from the origin, from the triangle's planes
                auto uv_at = [&](float x, float y, float& u, float& v) {
                    const RsWeights k = weights_at(at.c, x, y);
                    u = k(ta.uv[0], ta.uv[2], ta.uv[4]);
                    v = k(ta.uv[1], ta.uv[3], ta.uv[5]);
                };
                float u, v, u00, v00, u10, v10, u01, v01;
                uv_at(fx, fy, u, v);
                // the LOD's differences: the quad (global pixels) around this pixel, this pixel's triangle
                const float qx = (float)((int32_t)(gx & ~1u) - ox) + 0.5f, qy = (float)((int32_t)(gy & ~1u) - oy) + 0.5f;
                uv_at(qx, qy, u00, v00);
                uv_at(qx + 1.0f, qy, u10, v10);
                uv_at(qx, qy + 1.0f, u01, v01);
                const float dxu = u10 - u00, dxv = v10 - v00, dyu = u01 - u00, dyv = v01 - v00;
                float s[3];
                if (m.albedo != PBR_NO_MAP) {   // albedo = decode_gamma(sample.rgb): the encode applies decode_gamma
                    sample<3, BC1>(tl.tex[m.albedo], tl.dec, u, v, dxu, dxv, dyu, dyv, s);
                    a.x = s[0]; a.y = s[1]; a.z = s[2];
                }
                if (m.normal != PBR_NO_MAP) {   // sample_normal_texture; the encode's normalize is its normalize
                    const V3 n = normalize3_exact(v3(b.x, b.y, b.z));
                    const V3 tg = normalize3_exact(v3(l(ta.t[0], ta.t[3], ta.t[6]), l(ta.t[1], ta.t[4], ta.t[7]), l(ta.t[2], ta.t[5], ta.t[8])));
                    const V3 bt = cross3(n, tg);
                    sample<3, BC1>(tl.tex[m.normal], tl.dec, u, v, dxu, dxv, dyu, dyv, s);
                    const float tx_ = s[0] * 2.0f - 1.0f, ty_ = s[1] * 2.0f - 1.0f, tz_ = s[2] * 2.0f - 1.0f;
                    b.x = (tx_ * tg.x + ty_ * bt.x) + tz_ * n.x;
                    b.y = (tx_ * tg.y + ty_ * bt.y) + tz_ * n.y;
                    b.z = (tx_ * tg.z + ty_ * bt.z) + tz_ * n.z;
                }
                if (m.roughness != PBR_NO_MAP) {
                    sample<1, BC1>(tl.tex[m.roughness], tl.dec, u, v, dxu, dxv, dyu, dyv, s);
                    b.w = s[0];
                }
                if (m.metallic != PBR_NO_MAP) {
                    sample<1, BC1>(tl.tex[m.metallic], tl.dec, u, v, dxu, dxv, dyu, dyv, s);
                    c.x = s[0];
                }
                if (m.ao != PBR_NO_MAP) {
                    sample<1, BC1>(tl.tex[m.ao], tl.dec, u, v, dxu, dxv, dyu, dyv, s);
                    c.y = s[0];
                }
            }
        }
        PBR_GBUFFER_ENCODE(a, b, c, pa, pb, pc)
        qa = pa; qb = pb; qc = pc;
    }
    if (inside) {
        const size_t i = (size_t)ly * p.pitch + lx;
        A[i] = qa;
        B[i] = qb;
        C[i] = qc;
        depth[i] = zbuf;
        stencil[i] = (uint8_t)sten;
    }
}

// The depth-only raster: block = bin, lane = pixel, the depth in a register.  Per fragment the rule k_rs_raster applies
// (RS_FOR_EACH_FRAGMENT), then the minimum: the fragments of a pixel may come in any order, so the bin's list is walked as k_rs_fill_depth
// left it, from the pool, whatever its length: DEPTH_CHUNK raster records at a time are copied into LDS by all 256 lanes (16 bytes
// each, coalesced) and read from there by every lane at the same address, instead of one dependent scalar load from memory per
// triangle.  A wave holds four rows of the bin and skips a triangle whose pixel box (RsTri::lo / hi) misses them: a covered pixel's
// centre lies in a fan triangle, so inside the polygon's bounding box, so in the pixel box; the skip cannot change a bit.  A bin
// without a list (the pool was full) walks every triangle record and tests its box (every_record).
__global__ __launch_bounds__(256) void k_rs_depth(RsParams p, const uint32_t* __restrict__ hdr, const RsTri* __restrict__ tris,
                                                  const uint32_t* __restrict__ count, const uint32_t* __restrict__ offset,
                                                  const uint32_t* __restrict__ pool, float* __restrict__ depth) {
    __shared__ uint32_t list[256];
    __shared__ RsTri recs[DEPTH_CHUNK];
    static_assert(sizeof(RsTri) % sizeof(uint4) == 0 && alignof(RsTri) >= alignof(uint4), "raster records are copied 16 bytes at a time");
    constexpr uint32_t PARTS = sizeof(RsTri) / sizeof(uint4);
    const uint32_t tid = threadIdx.x;
    RS_BIN_PIXEL(p, tid);
    // the rows of this wave (global pixels): lanes 64 w .. 64 w + 63 are rows 4 w .. 4 w + 3 of the bin
    const uint32_t wy0 = p.y0 + blockIdx.y * BIN + (tid >> 6) * 4u, wy1 = wy0 + 3u;
    float zbuf = 1.0f;

    // one triangle (the same record for every lane of the block), unless its rows miss this wave's: the minimum, LESS without a winner
    auto fragment = [&](const RsTri& r) {
        if ((r.lo >> 16) > wy1 || (r.hi >> 16) < wy0) return;
        RS_FOR_EACH_FRAGMENT(r, z, if (z < zbuf) zbuf = z;)
    };

    const uint32_t b = blockIdx.y * p.nbx + blockIdx.x;
    const uint32_t cnt = count[b], off = offset[b];
    if (cnt != 0) {
        if (off != NONE) {
            for (uint32_t base = 0; base < cnt; base += DEPTH_CHUNK) {
                const uint32_t m = min(DEPTH_CHUNK, cnt - base);
                for (uint32_t q = tid; q < m * PARTS; q += 256u)
                    reinterpret_cast<uint4*>(recs)[q] = reinterpret_cast<const uint4*>(tris + pool[off + base + q / PARTS])[q % PARTS];
                __syncthreads();
                for (uint32_t j = 0; j < m; j++) fragment(recs[j]);
                __syncthreads();
            }
        } else {
            every_record(p, hdr, tris, list, tid, [&](uint32_t t) { fragment(tris[t]); });
        }
    }
    if (inside) depth[(size_t)ly * p.pitch + lx] = zbuf;
}

// the six planes of the model cull (pbr_hip.h) in fp64 from the fp32 matrices, each rounded once
void cull_planes(const pbr_global* g, const pbr_tile* tile, float* out) {
    double r[4][4];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            const float* P = g->Projection + 4 * i;
            const float* V = g->View + j;
            r[i][j] = (((double)P[0] * (double)V[0] + (double)P[1] * (double)V[4]) + (double)P[2] * (double)V[8]) + (double)P[3] * (double)V[12];
        }
    const double fw = (double)tile->full_w, fh = (double)tile->full_h;
    const double xl = 2.0 * ((double)tile->x0 - 1.0) / fw - 1.0;
    const double xr = 2.0 * (((double)tile->x0 + (double)tile->w) + 1.0) / fw - 1.0;
    const double yt = 1.0 - 2.0 * ((double)tile->y0 - 1.0) / fh;       // k_rs_setup's viewport: y = (1 - y_ndc) full_h / 2
    const double yb = 1.0 - 2.0 * (((double)tile->y0 + (double)tile->h) + 1.0) / fh;
    for (int j = 0; j < 4; j++) {
        out[0 + j] = (float)(r[0][j] - xl * r[3][j]);
        out[4 + j] = (float)(xr * r[3][j] - r[0][j]);
        out[8 + j] = (float)(r[1][j] - yb * r[3][j]);
        out[12 + j] = (float)(yt * r[3][j] - r[1][j]);
        out[16 + j] = (float)(r[3][j] + r[2][j]);
        out[20 + j] = (float)(r[3][j] - r[2][j]);
    }
}

// ---- the host side.  What the two descriptors share is exactly pbr_depth_raster_desc (pbr_raster_desc adds four planes and the
// texture fields): pbr_gbuffer_raster fills one from its own, and the checks, the parameters, the scratch carve and the first two
// launches take that. ----
using RsCall = pbr_depth_raster_desc;
static_assert(sizeof(pbr_raster_desc) == 152 && sizeof(pbr_depth_raster_desc) == 104, "descriptor layouts: no padding");

// What is wrong with the fields both entry points take (nullptr: nothing); the caller refuses under its own name (PBR_CHECK).
// own_null: one of the caller's other targets is null; own_addr: their addresses ORed, those that must be 4-byte aligned.
const char* cull_refusal(const RsCall& c) { return c.bounds || !c.stats ? nullptr : "stats without bounds"; }
const char* call_refusal(const RsCall& c, bool own_null, uintptr_t own_addr) {
    const pbr_tile* tile = c.tile;
    if (!(c.g && tile && c.vertices && c.indices && c.draws && c.depth && c.scratch) || own_null) return "null pointer";
    if (!(c.n_vertices && c.n_indices && c.n_draws && c.max_triangles)) return "empty vertex / index / draw list";
    if (!(c.n_draws <= PBR_RASTER_MAX_DRAWS && c.max_triangles <= PBR_RASTER_MAX_TRIANGLES)) return "more draws or triangles than the limits";
    if (!(tile->w && tile->h && tile->full_w && tile->full_h && tile->full_w <= PBR_RASTER_MAX_SIZE && tile->full_h <= PBR_RASTER_MAX_SIZE &&
          (uint64_t)tile->x0 + tile->w <= tile->full_w && (uint64_t)tile->y0 + tile->h <= tile->full_h))
        return "bad tile";
    if (!(c.pitch >= tile->w)) return "pitch < tile width";
    if (((pbr::addr(c.vertices) | pbr::addr(c.indices) | pbr::addr(c.draws) | pbr::addr(c.depth) | own_addr) & 3u) != 0 ||
        (pbr::addr(c.scratch) & 15u) != 0)
        return "unaligned buffer";
    if ((pbr::addr(c.bounds) & 3u) != 0) return "bounds not 4-byte aligned";
    if ((pbr::addr(c.stats) & 3u) != 0) return "stats not 4-byte aligned";
    return nullptr;
}

// the kernels' parameters of either chain; the pool is what the scratch holds past the layout's minimum
RsParams params(const RsCall& c, const Layout& L) {
    RsParams p;
    for (int i = 0; i < 16; i++) { p.View[i] = c.g->View[i]; p.Projection[i] = c.g->Projection[i]; }
    p.half_w = 0.5f * (float)c.tile->full_w;
    p.half_h = 0.5f * (float)c.tile->full_h;
    p.full_w = c.tile->full_w; p.full_h = c.tile->full_h;
    p.x0 = c.tile->x0; p.y0 = c.tile->y0; p.w = c.tile->w; p.h = c.tile->h;
    p.nbx = L.nbx;
    p.n_vertices = c.n_vertices; p.n_indices = c.n_indices; p.n_draws = c.n_draws;
    p.pitch = c.pitch;
    const size_t pool_entries = (c.scratch_bytes - L.pool) / 4;
    // (not min(): on the host HIP's min(size_t, size_t) is min(int, int), which made every capacity 0xfffffffe: no list was ever
    // refused for space, and a pool too small for the lists, the minimum scratch's empty one first of all, was written past its end)
    p.pool_cap = pool_entries < (size_t)0xfffffffeu ? (uint32_t)pool_entries : 0xfffffffeu;
    return p;
}

// the scratch, carved by its layout (attrs and tex: only where the layout has them), and the two grid sizes of a chain
struct Carve {
    uint32_t *hdr, *draw_base, *count, *cursor, *offset, *pool;
    RsTri* tris;
    RsAttr* attrs;
    RsTexAttr* tex;
    uint32_t n_bins, tri_blocks;
    Carve(const RsCall& c, const Layout& L) {
        char* s = static_cast<char*>(c.scratch);
        const auto words = [s](size_t at) { return reinterpret_cast<uint32_t*>(s + at); };
        hdr = words(0); draw_base = words(L.draw_base); count = words(L.count); cursor = words(L.cursor); offset = words(L.offset);
        pool = words(L.pool);
        tris = reinterpret_cast<RsTri*>(s + L.tris);
        attrs = reinterpret_cast<RsAttr*>(s + L.attrs);
        tex = reinterpret_cast<RsTexAttr*>(s + L.tex);
        n_bins = L.nbx * L.nby;
        tri_blocks = (c.max_triangles + 255u) / 256u;
    }
};

// the first two launches of either chain: k_rs_clear, and k_rs_prep with the model cull (c.bounds set: the planes are formed here) or without
pbr_status launch_clear_prep(pbr_ctx* ctx, const RsCall& c, const Carve& S) {
    hipLaunchKernelGGL(k_rs_clear, dim3(min((S.n_bins + 255u) / 256u, 1024u)), dim3(256), 0, ctx->stream, S.count, S.cursor, S.n_bins);
    if (pbr_status st = pbr::launched(ctx, "k_rs_clear")) return st;
    if (c.bounds) {
        RsCull cull{c.bounds, c.stats, {}};
        cull_planes(c.g, c.tile, cull.planes);
        hipLaunchKernelGGL(k_rs_prep<RsCull>, dim3(1), dim3(1024), 0, ctx->stream, c.draws, c.n_draws, c.max_triangles, S.draw_base, S.hdr, cull);
    } else {
        hipLaunchKernelGGL(k_rs_prep<>, dim3(1), dim3(1024), 0, ctx->stream, c.draws, c.n_draws, c.max_triangles, S.draw_base, S.hdr);
    }
    return pbr::launched(ctx, "k_rs_prep");
}

// pbr_gbuffer_raster: the checks and the six launches.  tx: null without d->maps, else the validated texture table (bc1: it holds a
// BC1-resident texture)
pbr_status raster(pbr_ctx* ctx, const pbr_raster_desc* d) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, d, "pbr_gbuffer_raster: null descriptor");
    const auto [g, tile, vertices, indices, draws, A, B, C, depth, stencil, scratch, scratch_bytes, maps, textures, bounds, stats,
                n_vertices, n_indices, n_draws, max_triangles, pitch, n_textures] = *d;
    const RsCall c{g, tile, vertices, indices, draws, depth, scratch, scratch_bytes, bounds, stats, n_vertices, n_indices, n_draws,
                   max_triangles, pitch, 0};
    PBR_REQUIRE(ctx, maps || (!textures && n_textures == 0), "pbr_gbuffer_raster: textures or n_textures without maps");
    PBR_CHECK(ctx, "pbr_gbuffer_raster", cull_refusal(c));
    RsRasterTex table;
    const RsRasterTex* tx = maps ? &table : nullptr;
    bool bc1 = false;
    if (tx) {
        PBR_REQUIRE(ctx, (pbr::addr(maps) & 3u) == 0, "pbr_gbuffer_raster: maps not 4-byte aligned");
        PBR_REQUIRE(ctx, n_textures <= PBR_RASTER_MAX_TEXTURES && (textures || n_textures == 0),
                    "pbr_gbuffer_raster: more textures than PBR_RASTER_MAX_TEXTURES, or a null texture table");
        table.maps = maps;
        table.tex = nullptr;
        table.n_tex = n_textures;
        for (uint32_t i = 0; i < PBR_RASTER_MAX_TEXTURES; i++) table.table[i] = pbr_texture2d{nullptr, 0, 0, 0, 0};
        for (uint32_t i = 0; i < n_textures; i++) {
            const pbr_texture2d& t = textures[i];
            PBR_CHECK(ctx, "pbr_gbuffer_raster", tex2d::refusal(t.width, t.height, t.mip_levels, t.format, true));
            PBR_REQUIRE(ctx, t.texels && tex2d::aligned(t.texels, t.format),
                        "pbr_gbuffer_raster: texels null or not aligned to the texel size (BC1 blocks: 8 bytes)");
            bc1 |= (t.format & PBR_TEX_BC1_BLOCKS) != 0;
            table.table[i] = t;
        }
    }
    PBR_CHECK(ctx, "pbr_gbuffer_raster", call_refusal(c, !(A && B && C && stencil), pbr::addr(A) | pbr::addr(B) | pbr::addr(C)));
    const Layout L = layout(tile->w, tile->h, max_triangles, tx != nullptr);
    PBR_REQUIRE(ctx, scratch_bytes >= L.pool, tx ? "pbr_gbuffer_raster: scratch below pbr_gbuffer_raster_textured_min_scratch_bytes"
                                                : "pbr_gbuffer_raster: scratch below pbr_gbuffer_raster_min_scratch_bytes");
    const RsParams p = params(c, L);
    const Carve S(c, L);

    if (pbr_status st = launch_clear_prep(ctx, c, S)) return st;
    if (tx) {
        const RsSetupTex st{tx->maps, S.tex, tx->n_tex};
        hipLaunchKernelGGL(k_rs_setup<RsSetupTex>, dim3(S.tri_blocks), dim3(256), 0, ctx->stream, p, vertices, indices, draws, S.draw_base,
                           S.hdr, S.tris, S.attrs, S.count, st);
    } else {
        hipLaunchKernelGGL(k_rs_setup<>, dim3(S.tri_blocks), dim3(256), 0, ctx->stream, p, vertices, indices, draws, S.draw_base, S.hdr,
                           S.tris, S.attrs, S.count);
    }
    if (pbr_status st = pbr::launched(ctx, "k_rs_setup")) return st;
    hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(64), 0, ctx->stream, S.count, S.n_bins, p.pool_cap, S.offset);
    if (pbr_status st = pbr::launched(ctx, "k_rs_scan")) return st;
    hipLaunchKernelGGL(k_rs_fill, dim3(S.tri_blocks), dim3(256), 0, ctx->stream, p, S.hdr, S.tris, S.offset, S.cursor, S.pool);
    if (pbr_status st = pbr::launched(ctx, "k_rs_fill")) return st;
    if (tx) {
        RsRasterTexBc1 rt;
        static_cast<RsRasterTex&>(rt) = *tx;
        rt.tex = S.tex;
        if (bc1)
            hipLaunchKernelGGL(k_rs_raster<RsRasterTexBc1>, dim3(L.nbx, L.nby), dim3(256), 0, ctx->stream, p, draws, S.hdr, S.tris, S.attrs,
                               S.count, S.offset, S.pool, A, B, C, depth, stencil, rt);
        else
            hipLaunchKernelGGL(k_rs_raster<RsRasterTex>, dim3(L.nbx, L.nby), dim3(256), 0, ctx->stream, p, draws, S.hdr, S.tris, S.attrs,
                               S.count, S.offset, S.pool, A, B, C, depth, stencil, static_cast<const RsRasterTex&>(rt));
    } else {
        hipLaunchKernelGGL(k_rs_raster<>, dim3(L.nbx, L.nby), dim3(256), 0, ctx->stream, p, draws, S.hdr, S.tris, S.attrs, S.count, S.offset,
                           S.pool, A, B, C, depth, stencil);
    }
    return pbr::launched(ctx, "k_rs_raster");
}

// pbr_depth_raster: pbr_gbuffer_raster's checks (without the planes it does not take) and the depth chain's six launches
pbr_status depth_raster(pbr_ctx* ctx, const pbr_depth_raster_desc* d) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, d, "pbr_depth_raster: null descriptor");
    const RsCall& c = *d;
    PBR_REQUIRE(ctx, c.reserved == 0, "pbr_depth_raster: reserved is not 0");
    PBR_CHECK(ctx, "pbr_depth_raster", cull_refusal(c));
    PBR_CHECK(ctx, "pbr_depth_raster", call_refusal(c, false, 0));
    const Layout L = layout(c.tile->w, c.tile->h, c.max_triangles, false, false);
    PBR_REQUIRE(ctx, c.scratch_bytes >= L.pool, "pbr_depth_raster: scratch below pbr_depth_raster_min_scratch_bytes");
    const RsParams p = params(c, L);
    const Carve S(c, L);

    if (pbr_status st = launch_clear_prep(ctx, c, S)) return st;
    hipLaunchKernelGGL(k_rs_setup<RsSetupDepth>, dim3(S.tri_blocks), dim3(256), 0, ctx->stream, p, c.vertices, c.indices, c.draws, S.draw_base,
                       S.hdr, S.tris, static_cast<RsAttr*>(nullptr), S.count, RsSetupDepth{});
    if (pbr_status st = pbr::launched(ctx, "k_rs_setup")) return st;
    hipLaunchKernelGGL(k_rs_scan_depth, dim3(1), dim3(1024), 0, ctx->stream, S.count, S.n_bins, p.pool_cap, S.offset);
    if (pbr_status st = pbr::launched(ctx, "k_rs_scan_depth")) return st;
    hipLaunchKernelGGL(k_rs_fill_depth, dim3(S.tri_blocks), dim3(256), 0, ctx->stream, p, S.hdr, S.tris, S.offset, S.cursor, S.pool);
    if (pbr_status st = pbr::launched(ctx, "k_rs_fill_depth")) return st;
    hipLaunchKernelGGL(k_rs_depth, dim3(L.nbx, L.nby), dim3(256), 0, ctx->stream, p, S.hdr, S.tris, S.count, S.offset, S.pool, c.depth);
    return pbr::launched(ctx, "k_rs_depth");
}

// the recommended scratch of a layout: its minimum and a pool of 8 entries per triangle and 4 per bin
size_t recommended(const Layout& L, uint32_t n_triangles) {
    return L.pool + align256(((size_t)8 * n_triangles + (size_t)4 * L.nbx * L.nby) * 4);
}

}  // namespace

extern "C" {

size_t pbr_gbuffer_raster_min_scratch_bytes(uint32_t w, uint32_t h, uint32_t n_triangles) { return layout(w, h, n_triangles).pool; }
size_t pbr_gbuffer_raster_scratch_bytes(uint32_t w, uint32_t h, uint32_t n_triangles) { return recommended(layout(w, h, n_triangles), n_triangles); }

size_t pbr_gbuffer_raster_textured_min_scratch_bytes(uint32_t w, uint32_t h, uint32_t n_triangles) { return layout(w, h, n_triangles, true).pool; }
size_t pbr_gbuffer_raster_textured_scratch_bytes(uint32_t w, uint32_t h, uint32_t n_triangles) {
    return recommended(layout(w, h, n_triangles, true), n_triangles);
}

pbr_status pbr_gbuffer_raster(pbr_ctx* ctx, const pbr_raster_desc* d) { return raster(ctx, d); }

size_t pbr_depth_raster_min_scratch_bytes(uint32_t w, uint32_t h, uint32_t n_triangles) { return layout(w, h, n_triangles, false, false).pool; }
size_t pbr_depth_raster_scratch_bytes(uint32_t w, uint32_t h, uint32_t n_triangles) {
    return recommended(layout(w, h, n_triangles, false, false), n_triangles);
}

pbr_status pbr_depth_raster(pbr_ctx* ctx, const pbr_depth_raster_desc* d) { return depth_raster(ctx, d); }

pbr_status pbr_draw_bounds(pbr_ctx* ctx, const pbr_vertex* vertices, uint32_t n_vertices, const uint32_t* indices, uint32_t n_indices,
                           const pbr_draw* draws, uint32_t n_draws, pbr_aabb* out) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, vertices && indices && draws && out, "pbr_draw_bounds: null pointer");
    PBR_REQUIRE(ctx, n_vertices && n_indices && n_draws && n_draws <= PBR_RASTER_MAX_DRAWS,
                "pbr_draw_bounds: empty vertex / index / draw list, or more draws than PBR_RASTER_MAX_DRAWS");
    PBR_REQUIRE(ctx, ((pbr::addr(vertices) | pbr::addr(indices) | pbr::addr(draws) | pbr::addr(out)) & 3u) == 0,
                "pbr_draw_bounds: unaligned buffer");
    hipLaunchKernelGGL(k_rs_bounds, dim3(n_draws), dim3(256), 0, ctx->stream, vertices, n_vertices, indices, n_indices, draws, out);
    return pbr::launched(ctx, "k_rs_bounds");
}

}  // extern "C"
