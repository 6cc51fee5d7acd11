// bc6h_encode_block.hpp — one lane of pbr_bc6h_encode_cube[_ex]: the BC6H_UF16 encoding rules pinned in include/pbr_hip.h (the one-region
// rule, and below it the two-region extension behind PBR_BC6H_ENCODE_TWO_REGION), from the lane's number to the 16 bytes of its block.  Plain C++ on integers (the one float operation is reading the texel): bc6h_encode.hip compiles
// it for gfx950, tools/bc6h_encode_hostcheck.cpp for the host, where the same text runs under ASan / UBSan against the restatement
// (tests/bc6h_encode_ref.py, tests/bc6h_encode2_ref.py).  No array here is indexed by a runtime value except through fully unrolled loops, so on the device
// everything stays in registers (no scratch); nothing is shared between lanes.  The one table read with a runtime index is the decode
// rule's PARTITION (constant memory), by the shape search's wave-uniform counter.
#pragma once
#include <cstdint>
#include <cstring>

#include "tex_chain.hpp"
#include "bc6h_decode_block.hpp"

#if defined(__HIPCC__)
#define BC6H_FN __host__ __device__ __forceinline__
#define BC6H2_FN __device__ __forceinline__                 // what uses the decode rule's tables: device only, as they are
#define BC6H_UNROLL _Pragma("unroll")
#define BC6H2_NOUNROLL _Pragma("nounroll")
#else
#define BC6H_FN inline
#define BC6H2_FN inline
#define BC6H_UNROLL
#define BC6H2_NOUNROLL
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

// ---- the two-region extension of the rule (PBR_BC6H_ENCODE_TWO_REGION) ----
// Everything above is the one-region rule and stays as it was, to the letter: k_bc6h_encode_cube compiles to the instructions it always had
// (factoring its start and its refinement out for the code below changed its register allocation, so the two are restated here over a
// texel mask and the 3-bit weights rather than shared).  The partition patterns, the anchors, the 3-bit weights and every header are the
// decode rule's own tables (bc6h_decode_block.hpp); the error of the one-region block is what that rule's per-texel form decodes of it.
constexpr uint64_t mode2_table(uint32_t what) {                        // a field of width 6 per two-region mode, in the order the rule tries them
    constexpr uint32_t order[10] = {0x00, 0x01, 0x02, 0x06, 0x0a, 0x0e, 0x12, 0x16, 0x1a, 0x1e};
    uint64_t v = 0;
    for (uint32_t i = 0; i < 10u; i++) {
        const bc6h_dec::ModeDesc d = bc6h_dec::mode_desc(order[i]);
        v |= (uint64_t)(what == 0u ? order[i] : what == 1u ? d.endpoint_bits : d.delta_bits[what - 2u]) << (6u * i);
    }
    return v;
}
constexpr uint64_t MODE2_NUMBER = mode2_table(0), MODE2_BITS = mode2_table(1);
constexpr uint64_t MODE2_DELTA[3] = {mode2_table(2), mode2_table(3), mode2_table(4)};

BC6H_FN uint32_t weight3(uint32_t k) { return (uint32_t)(bc6h_dec::WEIGHTS3 >> (8u * k)) & 255u; }
// a value that is the same in every lane, held as a scalar on the device
BC6H2_FN uint32_t uniform(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
#else
    return v;
#endif
}
BC6H_FN uint64_t nibbles(uint32_t mask) {                              // bit t -> 7 in nibble t
    uint64_t v = 0;
    BC6H_UNROLL
    for (uint32_t t = 0; t < 16u; t++) v |= ((mask >> t) & 1u) ? 7ull << (4u * t) : 0ull;
    return v;
}

// fit3: fit with the 3-bit weights and a pair per region.  e[6 r + 3 i + c]: region r's endpoint i (0: a, 1: b), channel c; pattern: bit t set
// for a texel of region 1.  idx: a nibble per texel, 0 outside the level; err[r]: region r's error
BC6H2_FN void fit3(const uint32_t (&h)[48], uint32_t valid, uint32_t pattern, const uint32_t (&e)[12], uint64_t& idx, uint64_t (&err)[2]) {
    uint32_t best[16], at[16];
    BC6H_UNROLL
    for (uint32_t t = 0; t < 16u; t++) { best[t] = 0xffffffffu; at[t] = 0u; }
    BC6H2_NOUNROLL
    for (uint32_t k = 0; k < 8u; k++) {                                // (a real loop, as in fit)
        const int32_t w = (int32_t)weight3(k);
        int32_t p[6];
        BC6H_UNROLL
        for (uint32_t j = 0; j < 6u; j++) {
            const uint32_t r = j / 3u, c = j - 3u * r;
            const int32_t ea = (int32_t)(e[6u * r + c] & 0xffffu), eb = (int32_t)(e[6u * r + 3u + c] & 0xffffu);
            const uint32_t x = (uint32_t)((ea << 6) + (eb - ea) * w + 32) >> 6;
            p[j] = (int32_t)((((x << 5) - x) >> 6) & 0x7fffu);
        }
        BC6H_UNROLL
        for (uint32_t t = 0; t < 16u; t++) {
            const bool second = (pattern >> t) & 1u;
            const int32_t dr = (second ? p[3] : p[0]) - (int32_t)h[3u * t], dg = (second ? p[4] : p[1]) - (int32_t)h[3u * t + 1u],
                          db = (second ? p[5] : p[2]) - (int32_t)h[3u * t + 2u];
            const uint32_t d = (uint32_t)(dr * dr) + (uint32_t)(dg * dg) + (uint32_t)(db * db);
            const bool less = d < best[t];                             // strictly: the lowest k keeps a tie
            best[t] = less ? d : best[t];
            at[t] = less ? k : at[t];
        }
    }
    idx = 0;
    err[0] = err[1] = 0;
    BC6H_UNROLL
    for (uint32_t t = 0; t < 16u; t++) {
        const bool in = (valid >> t) & 1u, second = (pattern >> t) & 1u;
        err[0] += in && !second ? best[t] : 0u;
        err[1] += in && second ? best[t] : 0u;
        idx |= in ? (uint64_t)at[t] << (4u * t) : 0ull;
    }
}

// the start of encode_block over the texels of `mask`; an empty mask gives 0, 0
BC6H_FN void box_start(const uint32_t (&h)[48], uint32_t mask, uint32_t (&A)[3], uint32_t (&B)[3]) {
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    uint64_t sum[3] = {0u, 0u, 0u};
    int64_t n = 0;
    BC6H_UNROLL
    for (uint32_t t = 0; t < 16u; t++) {
        const bool in = (mask >> t) & 1u;
        n += in ? 1 : 0;
        BC6H_UNROLL
        for (uint32_t c = 0; c < 3u; c++) {
            const uint32_t x = (64u * h[3u * t + c] + 30u) / 31u;
            lo[c] = in && x < lo[c] ? x : lo[c];
            hi[c] = in && x > hi[c] ? x : hi[c];
            sum[c] += in ? x : 0u;
        }
    }
    uint32_t dom = 0;
    if (hi[1] - lo[1] > hi[0] - lo[0]) dom = 1;
    if (hi[2] - lo[2] > (dom == 0u ? hi[0] - lo[0] : hi[1] - lo[1])) dom = 2;
    uint64_t sxd[3] = {0u, 0u, 0u};
    BC6H_UNROLL
    for (uint32_t t = 0; t < 16u; t++) {
        const uint32_t x0 = (64u * h[3u * t] + 30u) / 31u, x1 = (64u * h[3u * t + 1u] + 30u) / 31u, x2 = (64u * h[3u * t + 2u] + 30u) / 31u;
        const uint64_t xd = ((mask >> t) & 1u) ? (dom == 0u ? x0 : dom == 1u ? x1 : x2) : 0u;
        sxd[0] += x0 * xd; sxd[1] += x1 * xd; sxd[2] += x2 * xd;
    }
    const uint64_t sd = dom == 0u ? sum[0] : dom == 1u ? sum[1] : sum[2];
    BC6H_UNROLL
    for (uint32_t c = 0; c < 3u; c++) {
        const bool neg = n * (int64_t)sxd[c] - (int64_t)(sum[c] * sd) < 0;
        A[c] = mask == 0u ? 0u : neg ? lo[c] : hi[c];
        B[c] = mask == 0u ? 0u : neg ? hi[c] : lo[c];
    }
}
BC6H_FN void box_starts(const uint32_t (&h)[48], uint32_t valid, uint32_t pattern, uint32_t (&e)[12]) {
    BC6H_UNROLL
    for (uint32_t r = 0; r < 2u; r++) {
        uint32_t A[3], B[3];
        box_start(h, valid & (r == 0u ? ~pattern : pattern), A, B);
        BC6H_UNROLL
        for (uint32_t c = 0; c < 3u; c++) { e[6u * r + c] = A[c]; e[6u * r + 3u + c] = B[c]; }
    }
}

// the refinement step of encode_block for both regions at once, alpha and beta from the 3-bit weights.  One pass over the texels makes both
// regions' sums (a texel adds to its own region's; every sum fits 32 bits: alpha t < 2^22, sixteen of them); the endpoints then come out of a
// real loop over the regions, so the six divisions exist once.  can: bit r set where region r's system is not singular
BC6H_FN void least_squares3(const uint32_t (&h)[48], uint32_t valid, uint32_t pattern, uint64_t idx, uint32_t (&e2)[12], uint32_t& can) {
    uint32_t saa[2] = {0u, 0u}, sbb[2] = {0u, 0u}, sab[2] = {0u, 0u}, sat[6] = {0u, 0u, 0u, 0u, 0u, 0u}, sbt[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    BC6H_UNROLL
    for (uint32_t t = 0; t < 16u; t++) {
        const bool in = (valid >> t) & 1u, second = (pattern >> t) & 1u;
        const uint32_t be = weight3((uint32_t)(idx >> (4u * t)) & 7u), al = 64u - be;
        BC6H_UNROLL
        for (uint32_t r = 0; r < 2u; r++) {
            const bool on = in && second == (r == 1u);
            saa[r] += on ? al * al : 0u; sbb[r] += on ? be * be : 0u; sab[r] += on ? al * be : 0u;
            BC6H_UNROLL
            for (uint32_t c = 0; c < 3u; c++) {
                const uint32_t x = (64u * h[3u * t + c] + 30u) / 31u;
                sat[3u * r + c] += on ? al * x : 0u; sbt[3u * r + c] += on ? be * x : 0u;
            }
        }
    }
    can = 0;
    BC6H2_NOUNROLL
    for (uint32_t r = 0; r < 2u; r++) {
        const int64_t aa = r == 0u ? saa[0] : saa[1], bb = r == 0u ? sbb[0] : sbb[1], ab = r == 0u ? sab[0] : sab[1];
        const int64_t det = aa * bb - ab * ab;                         // >= 0 (Cauchy-Schwarz), below 2^33
        const int64_t dd = det == 0 ? 1 : det;                         // (a singular system's quotients are not used)
        can |= det != 0 ? 1u << r : 0u;
        BC6H_UNROLL
        for (uint32_t c = 0; c < 3u; c++) {                            // numerators below 2^50 in magnitude
            const int64_t at = r == 0u ? sat[c] : sat[3u + c], bt = r == 0u ? sbt[c] : sbt[3u + c];
            const int64_t qa = floor_div(128 * (bb * at - ab * bt) + dd, 2 * dd);
            const int64_t qb = floor_div(128 * (aa * bt - ab * at) + dd, 2 * dd);
            const uint32_t A2 = (uint32_t)(qa < 0 ? 0 : qa > 65535 ? 65535 : qa), B2 = (uint32_t)(qb < 0 ? 0 : qb > 65535 ? 65535 : qb);
            e2[c] = r == 0u ? A2 : e2[c];
            e2[3u + c] = r == 0u ? B2 : e2[3u + c];
            e2[6u + c] = r == 1u ? A2 : e2[6u + c];
            e2[9u + c] = r == 1u ? B2 : e2[9u + c];
        }
    }
}

// the squared error in half-code space of a block as the decode rule reads it, over the texels of `valid`
BC6H2_FN uint64_t decoded_error(const Block& b, const uint32_t (&h)[48], uint32_t valid) {
    const bc6h_dec::Block d = bc6h_dec::header(b.x, b.y, b.z, b.w);
    uint64_t err = 0;
    BC6H_UNROLL
    for (uint32_t t = 0; t < 16u; t++) {
        uint32_t half[3];
        bc6h_dec::texel(d, t, half);
        const int32_t dr = (int32_t)half[0] - (int32_t)h[3u * t], dg = (int32_t)half[1] - (int32_t)h[3u * t + 1u], db = (int32_t)half[2] - (int32_t)h[3u * t + 2u];
        err += ((valid >> t) & 1u) ? (uint32_t)(dr * dr) + (uint32_t)(dg * dg) + (uint32_t)(db * db) : 0u;
    }
    return err;
}

// the header of mode M from its stored fields f (r0 g0 b0 r1 ... b3, deltas already in two's complement of their width), through the
// decode rule's Seg table
template <uint32_t M, uint32_t S, uint32_t POS>
BC6H2_FN void write_header(const uint32_t (&f)[12], uint64_t& lo, uint64_t& hi) {
    constexpr bc6h_dec::ModeDesc D = bc6h_dec::mode_desc(M);
    if constexpr (S < D.count) {
        constexpr bc6h_dec::Seg g = D.segs[S];
        uint32_t v = (f[g.field] >> g.lo) & ((1u << g.n) - 1u);
        if constexpr (g.rev != 0) v = bc6h_dec::bit_reverse(v) >> (32u - g.n);
        if constexpr (POS >= 64u) hi |= (uint64_t)v << (POS - 64u);
        else {
            lo |= (uint64_t)v << POS;
            if constexpr (POS + g.n > 64u) hi |= (uint64_t)v >> (64u - POS);
        }
        write_header<M, S + 1u, POS + g.n>(f, lo, hi);
    }
}
template <uint32_t M>
BC6H2_FN void mode_header(const uint32_t (&f)[12], uint64_t& lo, uint64_t& hi) {
    lo = M;
    write_header<M, 0u, (M < 2u ? 2u : 5u)>(f, lo, hi);
}

// half codes of a block's texels (0 outside the level) -> the block of the two-region rule
BC6H2_FN Block encode_block2(const uint32_t (&h)[48], uint32_t valid) {
    const Block one = encode_block(h, valid);                          // step 1
    const uint64_t one_err = decoded_error(one, h, valid);
    if (one_err == 0u) return one;

    // step 3: the shape of least estimate.  s is the same in every lane, but the table's entries are 16 bits wide and there is no scalar
    // load of that width: the entry arrives through a vector load at a wave-uniform address and uniform() moves it into a scalar
    // register, which the per-texel region tests below take as a scalar operand.  The winner's pattern and number are carried along per lane
    uint32_t shape = 0, pattern = 0;
    uint64_t least = ~0ull;
    BC6H2_NOUNROLL
    for (uint32_t s = 0; s < 32u; s++) {
        const uint32_t pat = uniform(bc6h_dec::PARTITION[s]);
        uint32_t e[12];
        box_starts(h, valid, pat, e);
        uint64_t idx, err[2];
        fit3(h, valid, pat, e, idx, err);
        const bool take = err[0] + err[1] < least;                     // strictly: the lowest shape keeps a tie
        least = take ? err[0] + err[1] : least;
        shape = take ? s : shape;
        pattern = take ? pat : pattern;
    }

    // step 4: refine the two regions of that shape, each kept only while its own error falls
    const uint32_t in0 = valid & ~pattern, in1 = valid & pattern;
    const uint64_t nib1 = nibbles(in1);
    uint32_t e[12];
    box_starts(h, valid, pattern, e);
    uint64_t idx, err[2];
    fit3(h, valid, pattern, e, idx, err);
    bool going[2] = {true, true};
    BC6H2_NOUNROLL
    for (uint32_t it = 0; it < 2u; it++) {
        uint32_t e2[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, can;
        least_squares3(h, valid, pattern, idx, e2, can);
        BC6H_UNROLL
        for (uint32_t r = 0; r < 2u; r++) {                            // a region that has stopped, or is singular, keeps its pair
            going[r] = going[r] && ((can >> r) & 1u);
            BC6H_UNROLL
            for (uint32_t k = 0; k < 6u; k++) e2[6u * r + k] = going[r] ? e2[6u * r + k] : e[6u * r + k];
        }
        uint64_t idx2, err2[2];
        fit3(h, valid, pattern, e2, idx2, err2);
        BC6H_UNROLL
        for (uint32_t r = 0; r < 2u; r++) {
            going[r] = going[r] && err2[r] < err[r];
            const uint64_t mine = r == 0u ? ~nib1 : nib1;
            idx = going[r] ? (idx & ~mine) | (idx2 & mine) : idx;
            err[r] = going[r] ? err2[r] : err[r];
            BC6H_UNROLL
            for (uint32_t k = 0; k < 6u; k++) e[6u * r + k] = going[r] ? e2[6u * r + k] : e[6u * r + k];
        }
    }
    BC6H_UNROLL
    for (uint32_t k = 0; k < 6u; k++) e[6u + k] = in1 == 0u ? e[k] : e[6u + k];       // an empty region 1 takes region 0's pair

    // steps 5 and 6: the ten modes; the one-region block stays unless a candidate is strictly better, the earlier candidate keeps a tie
    const uint32_t anchor = shape < 16u ? 15u : (uint32_t)(bc6h_dec::ANCHOR_16_31 >> (4u * (shape - 16u))) & 15u;
    const uint64_t nib0 = nibbles(in0);
    uint32_t best_mode = 0xffu, best_q[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    uint64_t best_idx = 0, best_err = one_err;
    BC6H2_NOUNROLL
    for (uint32_t m = 0; m < 10u; m++) {
        const uint32_t bits = (uint32_t)(MODE2_BITS >> (6u * m)) & 63u;
        uint32_t q[12], u[12];
        BC6H_UNROLL
        for (uint32_t k = 0; k < 12u; k++) { q[k] = e[k] >> (16u - bits); u[k] = unquantize(q[k], bits); }
        uint64_t mi, me[2];
        fit3(h, valid, pattern, u, mi, me);
        BC6H_UNROLL
        for (uint32_t r = 0; r < 2u; r++) {                            // an anchor's high bit must be 0 (an anchor outside the level has index 0)
            const uint32_t a = r == 0u ? 0u : anchor;
            const bool flip = ((uint32_t)(mi >> (4u * a)) & 15u) >= 4u;
            BC6H_UNROLL
            for (uint32_t c = 0; c < 3u; c++) {
                const uint32_t qa = q[6u * r + c], qb = q[6u * r + 3u + c];
                q[6u * r + c] = flip ? qb : qa;
                q[6u * r + 3u + c] = flip ? qa : qb;
            }
            mi ^= flip ? (r == 0u ? nib0 : nib1) : 0ull;               // 7 - index, nibble by nibble
        }
        bool ok = true;
        if (m != 9u) {                                                 // 0x1e stores its endpoints as they are
            BC6H_UNROLL
            for (uint32_t c = 0; c < 3u; c++) {
                const int32_t half = 1 << (((uint32_t)(MODE2_DELTA[c] >> (6u * m)) & 63u) - 1u);
                BC6H_UNROLL
                for (uint32_t i = 1; i < 4u; i++) {
                    const int32_t d = (int32_t)q[3u * i + c] - (int32_t)q[c];
                    ok = ok && d >= -half && d < half;
                }
            }
        }
        const bool take = ok && me[0] + me[1] < best_err;
        best_err = take ? me[0] + me[1] : best_err;
        best_idx = take ? mi : best_idx;
        best_mode = take ? m : best_mode;
        BC6H_UNROLL
        for (uint32_t k = 0; k < 12u; k++) best_q[k] = take ? q[k] : best_q[k];
    }
    if (best_mode == 0xffu) return one;

    // step 7: the stored fields (e0 as it is, the others as deltas in two's complement of their width), the header through the decode
    // rule's table, the shape at bits 77 .. 81, the indices from bit 82: two bits for both anchors, three for the rest
    uint32_t f[12];
    BC6H_UNROLL
    for (uint32_t c = 0; c < 3u; c++) {
        const uint32_t dbits = (uint32_t)(MODE2_DELTA[c] >> (6u * best_mode)) & 63u;
        f[c] = best_q[c];
        BC6H_UNROLL
        for (uint32_t i = 1; i < 4u; i++) f[3u * i + c] = best_mode == 9u ? best_q[3u * i + c] : (best_q[3u * i + c] - best_q[c]) & ((1u << dbits) - 1u);
    }
    uint64_t lo64 = 0, hi64 = 0;
    switch ((uint32_t)(MODE2_NUMBER >> (6u * best_mode)) & 63u) {
        case 0x00: mode_header<0x00>(f, lo64, hi64); break;
        case 0x01: mode_header<0x01>(f, lo64, hi64); break;
        case 0x02: mode_header<0x02>(f, lo64, hi64); break;
        case 0x06: mode_header<0x06>(f, lo64, hi64); break;
        case 0x0a: mode_header<0x0a>(f, lo64, hi64); break;
        case 0x0e: mode_header<0x0e>(f, lo64, hi64); break;
        case 0x12: mode_header<0x12>(f, lo64, hi64); break;
        case 0x16: mode_header<0x16>(f, lo64, hi64); break;
        case 0x1a: mode_header<0x1a>(f, lo64, hi64); break;
        default:   mode_header<0x1e>(f, lo64, hi64); break;
    }
    hi64 |= (uint64_t)shape << 13;
    BC6H_UNROLL
    for (uint32_t t = 0; t < 16u; t++) {                               // (both anchors' third bit is 0: nothing runs into the next texel)
        const uint32_t start = 18u + 3u * t - (t > 0u ? 1u : 0u) - (t > anchor ? 1u : 0u);
        hi64 |= ((best_idx >> (4u * t)) & 7ull) << start;
    }
    return Block{(uint32_t)lo64, (uint32_t)(lo64 >> 32), (uint32_t)hi64, (uint32_t)(hi64 >> 32)};
}

// lane g of the launch: its level, face and block (the lanes of a level are face after face, a face's blocks row-major), the block's
// texels read from the cube chain, the block stored into its face's chain.  g < L.lanes.
template <bool TWO_REGION = false>
BC6H2_FN void encode_lane(const Cube& L, uint32_t g, const Texel* cube) {
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
    // (a conditional on the template constant, not `if constexpr`: with the latter — a declared-then-assigned Block, or a lambda around it —
    // the one-region kernel's loads are scheduled differently; clang emits only the live arm of a constant conditional either way)
    const Block b = TWO_REGION ? encode_block2(h, valid) : encode_block(h, valid);
    void* base = f == 0u ? L.face[0] : f == 1u ? L.face[1] : f == 2u ? L.face[2] : f == 3u ? L.face[3] : f == 4u ? L.face[4] : L.face[5];
    static_cast<Block*>(base)[ff + r] = b;
}

}  // namespace bc6h_enc
