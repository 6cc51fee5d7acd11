// bc6h_encode_block.hpp — one lane of pbr_bc6h_encode_cube: the BC6H_UF16 encoding rule pinned in include/pbr_hip.h, from the lane's
// number to the 16 bytes of its block.  Plain C++ on integers (the one float operation is reading the texel): bc6h_encode.hip compiles
// it for gfx950, tools/bc6h_encode_hostcheck.cpp for the host, where the same text runs under ASan / UBSan against the restatement
// (tests/bc6h_encode_ref.py).  No array here is indexed by a runtime value except through fully unrolled loops, so on the device
// everything stays in registers (no scratch); nothing is shared between lanes.
#pragma once
#include <cstdint>
#include <cstring>

#include "tex_chain.hpp"

#if defined(__HIPCC__)
#define BC6H_FN __host__ __device__ __forceinline__
#define BC6H_UNROLL _Pragma("unroll")
#else
#define BC6H_FN inline
#define BC6H_UNROLL
#endif

namespace bc6h_enc {

using bc6h_chain::MAX_LEVELS;
constexpr uint64_t WEIGHTS4_LO = 0x1e1a15110d090400ull;     // 0, 4, 9, 13, 17, 21, 26, 30: a byte each
constexpr uint64_t WEIGHTS4_HI = 0x403c37332f2b2622ull;     // 34, 38, 43, 47, 51, 55, 60, 64

struct alignas(16) Texel { float x, y, z, w; };                        // a float4 of the pbr_cube_f32 chain
struct alignas(16) Block { uint32_t x, y, z, w; };                     // 16 bytes, bit 0 of the block = bit 0 of x

using Cube = bc6h_chain::Cube<void*>;                                  // the launch's level table: bc6h_chain::fill makes it

BC6H_FN uint32_t weight(uint32_t k) {
    return (uint32_t)((k < 8u ? WEIGHTS4_LO : WEIGHTS4_HI) >> (8u * (k & 7u))) & 255u;
}

// the half bit pattern of clamp(v, 0, 65504), rounded to nearest even, in integers and without a branch: NaN and every v <= 0 (-0.0 too)
// give 0.  A positive float's bits order like its value, so the clamp is a minimum of bit patterns.
BC6H_FN uint32_t half_code(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    const bool zero = u - 1u >= 0x7f800000u;                           // +0.0, anything with the sign bit (-0.0, -NaN), +NaN; not +inf
    const uint32_t c = u < 0x477fe000u ? u : 0x477fe000u, e = c >> 23; // 65504 and above, +inf -> 65504
    const bool normal = e >= 113u;                                     // 2^-14 and above: rebias and drop 13 bits
    // a subnormal half is v * 2^24 = the 24-bit mantissa >> (126 - e), 14 bits and more (25: everything is shifted out, and 2^-25 ties to 0)
    const uint32_t x = normal ? c - (112u << 23) : (c & 0x7fffffu) | 0x800000u;
    const uint32_t sh = normal ? 13u : (126u - e < 25u ? 126u - e : 25u);
    const uint32_t h = (x + ((1u << (sh - 1u)) - 1u) + ((x >> sh) & 1u)) >> sh;      // to nearest even; a carry runs into the exponent, never past 0x7bff
    return zero ? 0u : h;
}

BC6H_FN uint32_t unquantize(uint32_t x, uint32_t n) {                  // the decode rule's, n = endpoint bits
    if (n >= 15u) return x;
    return x == 0u ? 0u : x == (1u << n) - 1u ? 0xffffu : ((x << 15) + 0x4000u) >> (n - 1u);
}

BC6H_FN int64_t floor_div(int64_t n, int64_t d) {                      // d > 0
    const int64_t q = n / d;
    return (n % d < 0) ? q - 1 : q;
}

// fit(a, b): per inside texel the palette entry of least squared distance in half-code space, the lowest index on ties.
// h[3 t + c]: the texels' half codes; valid: bit t set for a texel of the level.  idx: a nibble per texel, 0 for outside texels.
BC6H_FN void fit(const uint32_t (&h)[48], uint32_t valid, const uint32_t (&a)[3], const uint32_t (&b)[3], uint64_t& idx, uint64_t& err) {
    // (every product below is of factors the compiler can see to be within 24 bits — a, b and the half codes are masked where they
    // are made — so it is a full-rate 24-bit multiply, not a 32-bit one)
    uint32_t best[16], at[16];
    BC6H_UNROLL
    for (uint32_t t = 0; t < 16u; t++) { best[t] = 0xffffffffu; at[t] = 0u; }
    for (uint32_t k = 0; k < 16u; k++) {                               // (a real loop: sixteen copies of the body would not pay)
        const int32_t w = (int32_t)weight(k);
        int32_t p[3];
        BC6H_UNROLL
        for (uint32_t c = 0; c < 3u; c++) {                            // a (64 - w) + b w = 64 a + (b - a) w
            const int32_t ea = (int32_t)(a[c] & 0xffffu), eb = (int32_t)(b[c] & 0xffffu);
            const uint32_t x = (uint32_t)((ea << 6) + (eb - ea) * w + 32) >> 6;
            p[c] = (int32_t)((((x << 5) - x) >> 6) & 0x7fffu);         // x * 31 >> 6, at most 0x7bff
        }
        BC6H_UNROLL
        for (uint32_t t = 0; t < 16u; t++) {
            const int32_t dr = p[0] - (int32_t)h[3u * t], dg = p[1] - (int32_t)h[3u * t + 1u], db = p[2] - (int32_t)h[3u * t + 2u];
            const uint32_t d = (uint32_t)(dr * dr) + (uint32_t)(dg * dg) + (uint32_t)(db * db);     // each below 2^30, the sum below 2^32
            const bool less = d < best[t];                             // strictly: the lowest k keeps a tie
            best[t] = less ? d : best[t];
            at[t] = less ? k : at[t];
        }
    }
    idx = 0;
    err = 0;
    BC6H_UNROLL
    for (uint32_t t = 0; t < 16u; t++) {
        const bool in = (valid >> t) & 1u;
        err += in ? best[t] : 0u;
        idx |= in ? (uint64_t)at[t] << (4u * t) : 0ull;
    }
}

// half codes of a block's texels (0 outside the level) -> the block
BC6H_FN Block encode_block(const uint32_t (&h)[48], uint32_t valid) {
    // start: the box's corners in 16-bit endpoint space, paired per channel by the sign of its covariance with the widest channel
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    uint64_t sum[3] = {0u, 0u, 0u};
    int64_t n = 0;
    BC6H_UNROLL
    for (uint32_t t = 0; t < 16u; t++) {
        if ((valid >> t) & 1u) {
            n++;
            BC6H_UNROLL
            for (uint32_t c = 0; c < 3u; c++) {
                const uint32_t x = (64u * h[3u * t + c] + 30u) / 31u;
                lo[c] = x < lo[c] ? x : lo[c];
                hi[c] = x > hi[c] ? x : hi[c];
                sum[c] += x;
            }
        }
    }
    uint32_t dom = 0;
    if (hi[1] - lo[1] > hi[0] - lo[0]) dom = 1;
    if (hi[2] - lo[2] > (dom == 0u ? hi[0] - lo[0] : hi[1] - lo[1])) dom = 2;
    uint64_t sxd[3] = {0u, 0u, 0u};
    BC6H_UNROLL
    for (uint32_t t = 0; t < 16u; t++) {
        if ((valid >> t) & 1u) {
            const uint32_t x0 = (64u * h[3u * t] + 30u) / 31u, x1 = (64u * h[3u * t + 1u] + 30u) / 31u, x2 = (64u * h[3u * t + 2u] + 30u) / 31u;
            const uint64_t xd = dom == 0u ? x0 : dom == 1u ? x1 : x2;
            sxd[0] += x0 * xd; sxd[1] += x1 * xd; sxd[2] += x2 * xd;
        }
    }
    const uint64_t sd = dom == 0u ? sum[0] : dom == 1u ? sum[1] : sum[2];
    uint32_t A[3], B[3];
    BC6H_UNROLL
    for (uint32_t c = 0; c < 3u; c++) {
        const bool neg = n * (int64_t)sxd[c] - (int64_t)(sum[c] * sd) < 0;          // below 2^41 each
        A[c] = neg ? lo[c] : hi[c];
        B[c] = neg ? hi[c] : lo[c];
    }
    uint64_t idx, err;
    fit(h, valid, A, B, idx, err);

    // refine: the least-squares endpoints of the current indices, kept while the error falls
    bool going = true;
    for (uint32_t it = 0; it < 2u; it++) {
        int64_t saa = 0, sbb = 0, sab = 0, sat[3] = {0, 0, 0}, sbt[3] = {0, 0, 0};
        BC6H_UNROLL
        for (uint32_t t = 0; t < 16u; t++) {
            if ((valid >> t) & 1u) {
                const int64_t be = weight((uint32_t)(idx >> (4u * t)) & 15u), al = 64 - be;
                saa += al * al; sbb += be * be; sab += al * be;
                BC6H_UNROLL
                for (uint32_t c = 0; c < 3u; c++) {
                    const int64_t x = (64u * h[3u * t + c] + 30u) / 31u;
                    sat[c] += al * x; sbt[c] += be * x;
                }
            }
        }
        const int64_t det = saa * sbb - sab * sab;                     // >= 0 (Cauchy-Schwarz), below 2^33
        if (!going || det == 0) { going = false; continue; }
        uint32_t A2[3], B2[3];
        BC6H_UNROLL
        for (uint32_t c = 0; c < 3u; c++) {                            // numerators below 2^50 in magnitude
            const int64_t qa = floor_div(128 * (sbb * sat[c] - sab * sbt[c]) + det, 2 * det);
            const int64_t qb = floor_div(128 * (saa * sbt[c] - sab * sat[c]) + det, 2 * det);
            A2[c] = (uint32_t)(qa < 0 ? 0 : qa > 65535 ? 65535 : qa);
            B2[c] = (uint32_t)(qb < 0 ? 0 : qb > 65535 ? 65535 : qb);
        }
        uint64_t idx2, err2;
        fit(h, valid, A2, B2, idx2, err2);
        if (err2 < err) {
            BC6H_UNROLL
            for (uint32_t c = 0; c < 3u; c++) { A[c] = A2[c]; B[c] = B2[c]; }
            idx = idx2; err = err2;
        } else {
            going = false;
        }
    }

    // the four one-region modes, 16.4 first; the 16-bit mode's fit is the one just kept (unquantize is the identity there)
    uint64_t inside = 0;
    BC6H_UNROLL
    for (uint32_t t = 0; t < 16u; t++) inside |= ((valid >> t) & 1u) ? 15ull << (4u * t) : 0ull;
    uint32_t best_mode = 0, best_a[3] = {0u, 0u, 0u}, best_b[3] = {0u, 0u, 0u}, best_d = 0;
    uint64_t best_idx = 0, best_err = ~0ull;
    for (uint32_t m = 0; m < 4u; m++) {
        const uint32_t bits = m == 0u ? 16u : 13u - m, dbits = 20u - bits;             // 16.4, 12.8, 11.9, 10.10
        uint32_t qa[3], qb[3];
        BC6H_UNROLL
        for (uint32_t c = 0; c < 3u; c++) { qa[c] = A[c] >> (16u - bits); qb[c] = B[c] >> (16u - bits); }
        uint64_t mi = idx, me = err;
        if (m != 0u) {
            uint32_t ua[3], ub[3];
            BC6H_UNROLL
            for (uint32_t c = 0; c < 3u; c++) { ua[c] = unquantize(qa[c], bits); ub[c] = unquantize(qb[c], bits); }
            fit(h, valid, ua, ub, mi, me);
        }
        if (mi & 8u) {                                                 // texel 0's index >= 8: the anchor's high bit must be 0
            BC6H_UNROLL
            for (uint32_t c = 0; c < 3u; c++) { const uint32_t s = qa[c]; qa[c] = qb[c]; qb[c] = s; }
            mi = (0xffffffffffffffffull - mi) & inside;                // 15 - index, nibble by nibble (no borrow)
        }
        bool ok = true;
        if (m != 3u) {
            const int32_t half = 1 << (dbits - 1u);
            BC6H_UNROLL
            for (uint32_t c = 0; c < 3u; c++) {
                const int32_t d = (int32_t)qb[c] - (int32_t)qa[c];
                ok = ok && d >= -half && d < half;
            }
        }
        if (ok && me < best_err) {
            best_err = me; best_idx = mi; best_mode = m; best_d = dbits;
            BC6H_UNROLL
            for (uint32_t c = 0; c < 3u; c++) { best_a[c] = qa[c]; best_b[c] = qb[c]; }
        }
    }

    // emit: mode, r0 g0 b0 [9:0], then per channel a 10-bit group: the second endpoint (mode 0x03) or the delta in two's complement of
    // its width followed by the first endpoint's bits above 9, the HIGH bit first; then texel 0's 3 index bits and 15 x 4
    const uint32_t mode_bits = best_mode == 0u ? 0x0fu : best_mode == 1u ? 0x0bu : best_mode == 2u ? 0x07u : 0x03u;
    uint64_t lo64 = mode_bits, bit64 = 0;
    BC6H_UNROLL
    for (uint32_t c = 0; c < 3u; c++) {
        uint32_t group = best_b[c];
        if (best_mode != 3u) {
            const uint32_t top = best_a[c] >> 10, nt = 10u - best_d;   // nt bits above bit 9
            uint32_t rev = 0;
            BC6H_UNROLL
            for (uint32_t k = 0; k < 6u; k++) rev |= (k < nt && ((top >> k) & 1u)) ? 1u << (nt - 1u - k) : 0u;
            group = ((best_b[c] - best_a[c]) & ((1u << best_d) - 1u)) | (rev << best_d);
        }
        lo64 |= (uint64_t)(best_a[c] & 1023u) << (5u + 10u * c);
        lo64 |= (uint64_t)group << (35u + 10u * c);                    // (blue's tenth bit is block bit 64: shifted out here)
        if (c == 2u) bit64 = group >> 9;
    }
    const uint64_t hi64 = bit64 | ((best_idx & 7ull) << 1) | (best_idx & ~15ull);
    return Block{(uint32_t)lo64, (uint32_t)(lo64 >> 32), (uint32_t)hi64, (uint32_t)(hi64 >> 32)};
}

// lane g of the launch: its level, face and block (the lanes of a level are face after face, a face's blocks row-major), the block's
// texels read from the cube chain, the block stored into its face's chain.  g < L.lanes.
BC6H_FN void encode_lane(const Cube& L, uint32_t g, const Texel* cube) {
    uint32_t l = 0, ff = 0, ft = 0;
    BC6H_UNROLL
    for (uint32_t k = 1; k < MAX_LEVELS; k++) {                        // (static indices: the table stays in scalar registers)
        if (k < L.mips && g >= 6u * L.face_first[k]) { l = k; ff = L.face_first[k]; ft = L.first_texel[k]; }
    }
    const uint32_t s = L.size >> l, bw = s + 3u >= 4u ? (s + 3u) >> 2 : 1u, nb = bw * bw;
    const uint32_t k = g - 6u * ff, f = k / nb, r = k - f * nb, by = r / bw, bx = r - by * bw;
    const uint32_t nx = s - 4u * bx < 4u ? s - 4u * bx : 4u, ny = s - 4u * by < 4u ? s - 4u * by : 4u;
    const Texel* src = cube + ft + ((size_t)f * s + 4u * by) * s + 4u * bx;
    uint32_t h[48], valid = 0;
    BC6H_UNROLL
    for (uint32_t t = 0; t < 16u; t++) {
        const uint32_t x = t & 3u, y = t >> 2;
        const bool in = x < nx && y < ny;
        Texel q = {0.0f, 0.0f, 0.0f, 0.0f};
        if (in) q = src[(size_t)y * s + x];
        h[3u * t] = half_code(q.x) & 0x7fffu; h[3u * t + 1u] = half_code(q.y) & 0x7fffu; h[3u * t + 2u] = half_code(q.z) & 0x7fffu;     // (the mask: see fit)
        valid |= in ? 1u << t : 0u;
    }
    const Block b = encode_block(h, valid);
    void* base = f == 0u ? L.face[0] : f == 1u ? L.face[1] : f == 2u ? L.face[2] : f == 3u ? L.face[3] : f == 4u ? L.face[4] : L.face[5];
    static_cast<Block*>(base)[ff + r] = b;
}

}  // namespace bc6h_enc
