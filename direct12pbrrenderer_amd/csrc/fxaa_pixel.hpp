// fxaa_pixel.hpp — one pixel of pbr_fxaa: the anti-aliasing rule pinned in include/pbr_hip.h ("Anti-aliasing"), from the pixel's
// coordinates to its four output bytes, over a pixel fetcher.  Plain C++ on integers, nothing else: fxaa.hip compiles it for gfx950
// (its fetcher reads the block's LDS tile and, beyond it, global memory), tools/fxaa_hostcheck.cpp for the host, where the same text
// runs under ASan / UBSan against the restatement (tests/fxaa_ref.py).
//   A fetcher F has   uint32_t rgba(int x, int y) const   and   int luma(int x, int y) const   for 0 <= x < w, 0 <= y < h; the rule
// clamps every coordinate before it asks, so a fetcher never sees one outside the image.
// Every intermediate fits 32 bits: a luma is at most 65 280, 256 * |A - 12 M| at most 256 * 12 * 65 280 < 2^28, t * t * (768 - 2 t) at
// most 2^24.  Both divisors are positive: an edge pixel's range is at least EDGE_MIN, and kn + kp at least 2.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define FXAA_FN __host__ __device__ __forceinline__
#else
#define FXAA_FN inline
#endif

namespace fxaa {

constexpr int EDGE_MIN = 4080;       // 16 grey levels of luma
constexpr int WALK_LAST = 24;        // the farthest offset of the walk: the rule reads up to 24 pixels along the edge and 1 across
// the walk's offsets 1 .. 8, 10, 12, 14, 16, 20, 24 without a table: the step grows from 1 to 2 after 8 and to 4 after 16
FXAA_FN int walk_step(int k) { return k < 8 ? 1 : k < 16 ? 2 : 4; }

FXAA_FN int luma_of(uint32_t p) { return 77 * (int)(p & 255u) + 150 * (int)((p >> 8) & 255u) + 29 * (int)((p >> 16) & 255u); }
FXAA_FN int iabs(int v) { return v < 0 ? -v : v; }
FXAA_FN int imin(int a, int b) { return a < b ? a : b; }
FXAA_FN int imax(int a, int b) { return a > b ? a : b; }
FXAA_FN int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// the contrast test: is (x, y) an edge pixel
template <class F>
FXAA_FN bool is_edge(const F& f, int x, int y, int w, int h) {
    const int xl = imax(x - 1, 0), xr = imin(x + 1, w - 1), yu = imax(y - 1, 0), yd = imin(y + 1, h - 1);
    const int m = f.luma(x, y), n = f.luma(x, yu), s = f.luma(x, yd), we = f.luma(xl, y), e = f.luma(xr, y);
    const int hi = imax(imax(imax(m, n), imax(s, we)), e), lo = imin(imin(imin(m, n), imin(s, we)), e);
    return hi - lo >= imax(EDGE_MIN, hi >> 3);
}

// one direction of the walk: d = -1 or +1 along (ax, ay); (cx, cy) is the step to the chosen side
template <class F>
FXAA_FN void walk(const F& f, int x, int y, int w, int h, int d, int ax, int ay, int cx, int cy, int p2, int g, int& k_end, int& e_end) {
    int k = 1, e = 0;
    for (;;) {
        const int mx = clampi(x + d * k * ax, w - 1), my = clampi(y + d * k * ay, h - 1);
        e = f.luma(mx, my) + f.luma(clampi(mx + cx, w - 1), clampi(my + cy, h - 1)) - p2;
        if (2 * iabs(e) >= g || k == WALK_LAST) break;
        k += walk_step(k);
    }
    k_end = k;
    e_end = e;
}

// the filtered value of a pixel that passed the contrast test
template <class F>
FXAA_FN uint32_t filter_edge(const F& f, int x, int y, int w, int h) {
    const int xl = imax(x - 1, 0), xr = imin(x + 1, w - 1), yu = imax(y - 1, 0), yd = imin(y + 1, h - 1);
    const int m = f.luma(x, y), n = f.luma(x, yu), s = f.luma(x, yd), we = f.luma(xl, y), e = f.luma(xr, y);
    const int nw = f.luma(xl, yu), ne = f.luma(xr, yu), sw = f.luma(xl, yd), se = f.luma(xr, yd);
    const int hi = imax(imax(imax(m, n), imax(s, we)), e), lo = imin(imin(imin(m, n), imin(s, we)), e);
    const int range = hi - lo;
    const int eh = iabs(nw + sw - 2 * we) + 2 * iabs(n + s - 2 * m) + iabs(ne + se - 2 * e);
    const int ev = iabs(nw + ne - 2 * n) + 2 * iabs(we + e - 2 * m) + iabs(sw + se - 2 * s);
    const bool horz = eh >= ev;
    const int a = horz ? n : we, b = horz ? s : e;
    const int da = iabs(a - m), db = iabs(b - m);
    const bool side_a = da >= db;
    const int g = side_a ? da : db, step = side_a ? -1 : 1;
    const int ax = horz ? 1 : 0, ay = horz ? 0 : 1, cx = horz ? 0 : step, cy = horz ? step : 0;
    const int nx = clampi(x + cx, w - 1), ny = clampi(y + cy, h - 1);
    const int nb = side_a ? a : b;
    const int p2 = m + nb;
    const bool m_lt = m < nb;
    int kn, en, kp, ep;
    walk(f, x, y, w, h, -1, ax, ay, cx, cy, p2, g, kn, en);
    walk(f, x, y, w, h, +1, ax, ay, cx, cy, p2, g, kp, ep);
    const bool first = kn < kp;
    const int dst = first ? kn : kp;
    const bool good = ((first ? en : ep) < 0) != m_lt;
    const int off8 = good ? 128 - (256 * dst) / (kn + kp) : 0;
    const int amount = iabs(2 * (n + s + we + e) + nw + ne + sw + se - 12 * m);
    const int t = imin(256, (int)((uint32_t)(256 * amount) / (uint32_t)(12 * range)));
    const int sm = (t * t * (768 - 2 * t)) >> 16;
    const int sub8 = (3 * sm * sm) >> 10;
    const uint32_t f8 = (uint32_t)imax(off8, sub8), r8 = 256u - f8;
    const uint32_t pm = f.rgba(x, y), pn = f.rgba(nx, ny);
    uint32_t out = pm & 0xff000000u;
    out |= ((pm & 255u) * r8 + (pn & 255u) * f8 + 128u) >> 8;
    out |= ((((pm >> 8) & 255u) * r8 + ((pn >> 8) & 255u) * f8 + 128u) >> 8) << 8;
    out |= ((((pm >> 16) & 255u) * r8 + ((pn >> 16) & 255u) * f8 + 128u) >> 8) << 16;
    return out;
}

template <class F>
FXAA_FN uint32_t pixel(const F& f, int x, int y, int w, int h) {
    return is_edge(f, x, y, w, h) ? filter_edge(f, x, y, w, h) : f.rgba(x, y);
}

// the fetcher of an image in plain memory (pitch in pixels): the host check's, and the kernel's beyond its LDS tile
struct MemoryFetch {
    const uint32_t* px;
    uint32_t pitch;
    FXAA_FN uint32_t rgba(int x, int y) const { return px[(size_t)y * pitch + (size_t)x]; }
    FXAA_FN int luma(int x, int y) const { return luma_of(rgba(x, y)); }
};

}  // namespace fxaa
