// bc6h_decode_block.hpp — the BC6H_UF16 decode rule pinned in include/pbr_hip.h in the two forms its users need:
//   per block   the mode tables, read_header / endpoints<M>, and the two steps both forms share — mode_endpoints() (the mode
//               switch) and texel_weight() —: k_bc6h_decode_cube (bc6h_decode.hip) expands whole blocks with them
//   per texel   header(): the 16 bytes of a block -> a Block (its unquantized endpoints packed two to a word, the index word, the
//               partition pattern and anchor); texel(): a Block and a texel number -> three half codes; half_to_f32(): the fp32 value.
//               The in-place sky resolve (k_skybox_bc6h, raster.hip) runs header() once per distinct block of a footprint and texel()
//               per tap.
// Plain C++ on integers: hipcc compiles it for gfx950, tools/bc6h_texel_hostcheck.cpp for the host, where the same text runs under
// ASan / UBSan against the restatement (tests/bc6h_ref.py).  No array here is indexed by a runtime value except PARTITION (constant
// memory on the device): the twelve endpoints are reached through static indices and selects, so everything stays in registers.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define BC6H_DEC_FN __device__ __forceinline__
#define BC6H_DEC_UNROLL _Pragma("unroll")
#define BC6H_DEC_TABLE static __constant__      // read by device code only: it stays local to the code object
#else
#define BC6H_DEC_FN inline
#define BC6H_DEC_UNROLL
#define BC6H_DEC_TABLE static const
#endif

// texel t in bit t: set = the second endpoint pair (e2 / e3).  In an unnamed namespace of the including file, where k_bc6h_decode_cube has always
// kept it: the table's symbol, and with it every line of that kernel, stays what it was.
namespace {
BC6H_DEC_TABLE uint16_t PARTITION[32] = {0xcccc, 0x8888, 0xeeee, 0xecc8, 0xc880, 0xfeec, 0xfec8, 0xec80, 0xc800, 0xffec, 0xfe80,
                                         0xe800, 0xffe8, 0xff00, 0xfff0, 0xf000, 0xf710, 0x008e, 0x7100, 0x08ce, 0x008c, 0x7310,
                                         0x3100, 0x8cce, 0x088c, 0x3110, 0x6666, 0x366c, 0x17e8, 0x0ff0, 0x718e, 0x399c};
}  // namespace

namespace bc6h_dec {

// ---- the header of every mode: its fields in file order (LSB first), after the mode bits ----
enum : uint8_t { R0, G0, B0, R1, G1, B1, R2, G2, B2, R3, G3, B3 };
// n file bits -> bits lo .. lo + n - 1 of a field, the lowest first (rev: the highest first)
struct Seg { uint8_t field, lo, n, rev; };
constexpr Seg H00[] = {{G2, 4, 1, 0}, {B2, 4, 1, 0}, {B3, 4, 1, 0}, {R0, 0, 10, 0}, {G0, 0, 10, 0}, {B0, 0, 10, 0}, {R1, 0, 5, 0}, {G3, 4, 1, 0}, {G2, 0, 4, 0}, {G1, 0, 5, 0}, {B3, 0, 1, 0}, {G3, 0, 4, 0}, {B1, 0, 5, 0}, {B3, 1, 1, 0}, {B2, 0, 4, 0}, {R2, 0, 5, 0}, {B3, 2, 1, 0}, {R3, 0, 5, 0}, {B3, 3, 1, 0}};
constexpr Seg H01[] = {{G2, 5, 1, 0}, {G3, 4, 2, 0}, {R0, 0, 7, 0}, {B3, 0, 2, 0}, {B2, 4, 1, 0}, {G0, 0, 7, 0}, {B2, 5, 1, 0}, {B3, 2, 1, 0}, {G2, 4, 1, 0}, {B0, 0, 7, 0}, {B3, 3, 1, 0}, {B3, 4, 2, 1}, {R1, 0, 6, 0}, {G2, 0, 4, 0}, {G1, 0, 6, 0}, {G3, 0, 4, 0}, {B1, 0, 6, 0}, {B2, 0, 4, 0}, {R2, 0, 6, 0}, {R3, 0, 6, 0}};
constexpr Seg H02[] = {{R0, 0, 10, 0}, {G0, 0, 10, 0}, {B0, 0, 10, 0}, {R1, 0, 5, 0}, {R0, 10, 1, 0}, {G2, 0, 4, 0}, {G1, 0, 4, 0}, {G0, 10, 1, 0}, {B3, 0, 1, 0}, {G3, 0, 4, 0}, {B1, 0, 4, 0}, {B0, 10, 1, 0}, {B3, 1, 1, 0}, {B2, 0, 4, 0}, {R2, 0, 5, 0}, {B3, 2, 1, 0}, {R3, 0, 5, 0}, {B3, 3, 1, 0}};
constexpr Seg H06[] = {{R0, 0, 10, 0}, {G0, 0, 10, 0}, {B0, 0, 10, 0}, {R1, 0, 4, 0}, {R0, 10, 1, 0}, {G3, 4, 1, 0}, {G2, 0, 4, 0}, {G1, 0, 5, 0}, {G0, 10, 1, 0}, {G3, 0, 4, 0}, {B1, 0, 4, 0}, {B0, 10, 1, 0}, {B3, 1, 1, 0}, {B2, 0, 4, 0}, {R2, 0, 4, 0}, {B3, 0, 1, 0}, {B3, 2, 1, 0}, {R3, 0, 4, 0}, {G2, 4, 1, 0}, {B3, 3, 1, 0}};
constexpr Seg H0A[] = {{R0, 0, 10, 0}, {G0, 0, 10, 0}, {B0, 0, 10, 0}, {R1, 0, 4, 0}, {R0, 10, 1, 0}, {B2, 4, 1, 0}, {G2, 0, 4, 0}, {G1, 0, 4, 0}, {G0, 10, 1, 0}, {B3, 0, 1, 0}, {G3, 0, 4, 0}, {B1, 0, 5, 0}, {B0, 10, 1, 0}, {B2, 0, 4, 0}, {R2, 0, 4, 0}, {B3, 1, 2, 0}, {R3, 0, 4, 0}, {B3, 3, 2, 1}};
constexpr Seg H0E[] = {{R0, 0, 9, 0}, {B2, 4, 1, 0}, {G0, 0, 9, 0}, {G2, 4, 1, 0}, {B0, 0, 9, 0}, {B3, 4, 1, 0}, {R1, 0, 5, 0}, {G3, 4, 1, 0}, {G2, 0, 4, 0}, {G1, 0, 5, 0}, {B3, 0, 1, 0}, {G3, 0, 4, 0}, {B1, 0, 5, 0}, {B3, 1, 1, 0}, {B2, 0, 4, 0}, {R2, 0, 5, 0}, {B3, 2, 1, 0}, {R3, 0, 5, 0}, {B3, 3, 1, 0}};
constexpr Seg H12[] = {{R0, 0, 8, 0}, {G3, 4, 1, 0}, {B2, 4, 1, 0}, {G0, 0, 8, 0}, {B3, 2, 1, 0}, {G2, 4, 1, 0}, {B0, 0, 8, 0}, {B3, 3, 2, 0}, {R1, 0, 6, 0}, {G2, 0, 4, 0}, {G1, 0, 5, 0}, {B3, 0, 1, 0}, {G3, 0, 4, 0}, {B1, 0, 5, 0}, {B3, 1, 1, 0}, {B2, 0, 4, 0}, {R2, 0, 6, 0}, {R3, 0, 6, 0}};
constexpr Seg H16[] = {{R0, 0, 8, 0}, {B3, 0, 1, 0}, {B2, 4, 1, 0}, {G0, 0, 8, 0}, {G2, 4, 2, 1}, {B0, 0, 8, 0}, {G3, 5, 1, 0}, {B3, 4, 1, 0}, {R1, 0, 5, 0}, {G3, 4, 1, 0}, {G2, 0, 4, 0}, {G1, 0, 6, 0}, {G3, 0, 4, 0}, {B1, 0, 5, 0}, {B3, 1, 1, 0}, {B2, 0, 4, 0}, {R2, 0, 5, 0}, {B3, 2, 1, 0}, {R3, 0, 5, 0}, {B3, 3, 1, 0}};
constexpr Seg H1A[] = {{R0, 0, 8, 0}, {B3, 1, 1, 0}, {B2, 4, 1, 0}, {G0, 0, 8, 0}, {B2, 5, 1, 0}, {G2, 4, 1, 0}, {B0, 0, 8, 0}, {B3, 4, 2, 1}, {R1, 0, 5, 0}, {G3, 4, 1, 0}, {G2, 0, 4, 0}, {G1, 0, 5, 0}, {B3, 0, 1, 0}, {G3, 0, 4, 0}, {B1, 0, 6, 0}, {B2, 0, 4, 0}, {R2, 0, 5, 0}, {B3, 2, 1, 0}, {R3, 0, 5, 0}, {B3, 3, 1, 0}};
constexpr Seg H1E[] = {{R0, 0, 6, 0}, {G3, 4, 1, 0}, {B3, 0, 2, 0}, {B2, 4, 1, 0}, {G0, 0, 6, 0}, {G2, 5, 1, 0}, {B2, 5, 1, 0}, {B3, 2, 1, 0}, {G2, 4, 1, 0}, {B0, 0, 6, 0}, {G3, 5, 1, 0}, {B3, 3, 1, 0}, {B3, 4, 2, 1}, {R1, 0, 6, 0}, {G2, 0, 4, 0}, {G1, 0, 6, 0}, {G3, 0, 4, 0}, {B1, 0, 6, 0}, {B2, 0, 4, 0}, {R2, 0, 6, 0}, {R3, 0, 6, 0}};
constexpr Seg H03[] = {{R0, 0, 10, 0}, {G0, 0, 10, 0}, {B0, 0, 10, 0}, {R1, 0, 10, 0}, {G1, 0, 10, 0}, {B1, 0, 10, 0}};
constexpr Seg H07[] = {{R0, 0, 10, 0}, {G0, 0, 10, 0}, {B0, 0, 10, 0}, {R1, 0, 9, 0}, {R0, 10, 1, 0}, {G1, 0, 9, 0}, {G0, 10, 1, 0}, {B1, 0, 9, 0}, {B0, 10, 1, 0}};
constexpr Seg H0B[] = {{R0, 0, 10, 0}, {G0, 0, 10, 0}, {B0, 0, 10, 0}, {R1, 0, 8, 0}, {R0, 10, 2, 1}, {G1, 0, 8, 0}, {G0, 10, 2, 1}, {B1, 0, 8, 0}, {B0, 10, 2, 1}};
constexpr Seg H0F[] = {{R0, 0, 10, 0}, {G0, 0, 10, 0}, {B0, 0, 10, 0}, {R1, 0, 4, 0}, {R0, 10, 6, 1}, {G1, 0, 4, 0}, {G0, 10, 6, 1}, {B1, 0, 4, 0}, {B0, 10, 6, 1}};

struct ModeDesc {
    uint32_t endpoint_bits, delta_bits[3];
    bool transformed, two;
    const Seg* segs;
    uint32_t count;
};
template <uint32_t N>
constexpr ModeDesc mode_of(uint32_t nb, uint32_t dr, uint32_t dg, uint32_t db, bool transformed, bool two, const Seg (&s)[N]) {
    return ModeDesc{nb, {dr, dg, db}, transformed, two, s, N};
}
constexpr ModeDesc mode_desc(uint32_t mode) {
    switch (mode) {
        case 0x00: return mode_of(10, 5, 5, 5, true, true, H00);
        case 0x01: return mode_of(7, 6, 6, 6, true, true, H01);
        case 0x02: return mode_of(11, 5, 4, 4, true, true, H02);
        case 0x06: return mode_of(11, 4, 5, 4, true, true, H06);
        case 0x0a: return mode_of(11, 4, 4, 5, true, true, H0A);
        case 0x0e: return mode_of(9, 5, 5, 5, true, true, H0E);
        case 0x12: return mode_of(8, 6, 5, 5, true, true, H12);
        case 0x16: return mode_of(8, 5, 6, 5, true, true, H16);
        case 0x1a: return mode_of(8, 5, 5, 6, true, true, H1A);
        case 0x1e: return mode_of(6, 6, 6, 6, false, true, H1E);
        case 0x03: return mode_of(10, 10, 10, 10, false, false, H03);
        case 0x07: return mode_of(11, 9, 9, 9, true, false, H07);
        case 0x0b: return mode_of(12, 8, 8, 8, true, false, H0B);
        default:   return mode_of(16, 4, 4, 4, true, false, H0F);     // 0x0f
    }
}
constexpr uint32_t header_end(uint32_t mode) {
    const ModeDesc d = mode_desc(mode);
    uint32_t pos = mode < 2 ? 2 : 5;
    for (uint32_t i = 0; i < d.count; i++) pos += d.segs[i].n;
    return pos;
}
static_assert(header_end(0x00) == 77 && header_end(0x01) == 77 && header_end(0x02) == 77 && header_end(0x06) == 77 && header_end(0x0a) == 77 &&
              header_end(0x0e) == 77 && header_end(0x12) == 77 && header_end(0x16) == 77 && header_end(0x1a) == 77 && header_end(0x1e) == 77,
              "a two-region header ends where the partition starts");
static_assert(header_end(0x03) == 65 && header_end(0x07) == 65 && header_end(0x0b) == 65 && header_end(0x0f) == 65,
              "a one-region header ends where the indices start");

using ::PARTITION;
constexpr uint64_t ANCHOR_16_31 = 0x22882282f882282full;      // region 1's anchor texel of shapes 16 .. 31, a nibble each (0 .. 15: 15)
constexpr uint64_t WEIGHTS3 = 0x40372e251b120900ull;          // 0, 9, 18, 27, 37, 46, 55, 64: a byte each
constexpr uint64_t WEIGHTS4_LO = 0x1e1a15110d090400ull;       // 0, 4, 9, 13, 17, 21, 26, 30
constexpr uint64_t WEIGHTS4_HI = 0x403c37332f2b2622ull;       // 34, 38, 43, 47, 51, 55, 60, 64

BC6H_DEC_FN uint32_t bit_reverse(uint32_t v) {
#if defined(__clang__)
    return __builtin_bitreverse32(v);
#else
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    return (v >> 16) | (v << 16);
#endif
}
// bits POS .. POS + N - 1 of the block
template <uint32_t POS, uint32_t N>
BC6H_DEC_FN uint32_t block_bits(uint64_t lo, uint64_t hi) {
    static_assert(N >= 1 && N <= 16 && POS + N <= 128, "a header field");
    uint64_t v;
    if constexpr (POS >= 64) v = hi >> (POS - 64);
    else if constexpr (POS + N <= 64) v = lo >> POS;
    else v = (lo >> POS) | (hi << (64 - POS));
    return (uint32_t)v & ((1u << N) - 1u);
}
template <uint32_t M, uint32_t S, uint32_t POS>
BC6H_DEC_FN void read_header(uint64_t lo, uint64_t hi, uint32_t (&e)[12]) {
    constexpr ModeDesc D = mode_desc(M);
    if constexpr (S < D.count) {
        constexpr Seg g = D.segs[S];
        uint32_t v = block_bits<POS, g.n>(lo, hi);
        if constexpr (g.rev != 0) v = bit_reverse(v) >> (32u - g.n);
        e[g.field] |= v << g.lo;
        read_header<M, S + 1, POS + g.n>(lo, hi, e);
    }
}
template <uint32_t N>
BC6H_DEC_FN uint32_t unquantize(uint32_t x) {
    if constexpr (N >= 15) return x;
    else return x == 0u ? 0u : x == (1u << N) - 1u ? 0xffffu : ((x << 15) + 0x4000u) >> (N - 1u);
}
// a mode's header -> its unquantized endpoints e[3 i + c] (i: e0 .. e3, c: r, g, b); one-region modes leave e2 / e3 zero
template <uint32_t M>
BC6H_DEC_FN void endpoints(uint64_t lo, uint64_t hi, uint32_t (&e)[12]) {
    constexpr ModeDesc D = mode_desc(M);
    read_header<M, 0, (M < 2 ? 2u : 5u)>(lo, hi, e);
    constexpr uint32_t mask = (1u << D.endpoint_bits) - 1u, last = D.two ? 3u : 1u;
    if constexpr (D.transformed) {
        BC6H_DEC_UNROLL
        for (uint32_t i = 1; i <= last; i++) {
            BC6H_DEC_UNROLL
            for (uint32_t c = 0; c < 3u; c++) {
                const uint32_t sh = 32u - D.delta_bits[c];
                e[3u * i + c] = (e[c] + (uint32_t)((int32_t)(e[3u * i + c] << sh) >> sh)) & mask;
            }
        }
    }
    BC6H_DEC_UNROLL
    for (uint32_t k = 0; k < 3u * (last + 1u); k++) e[k] = unquantize<D.endpoint_bits>(e[k]);
}

// the mode switch: the block's header -> e (zero on entry) by its mode's rule; returns whether the mode has two regions
BC6H_DEC_FN bool mode_endpoints(uint64_t lo, uint64_t hi, uint32_t (&e)[12]) {
    const uint32_t x = (uint32_t)lo, mode = (x & 2u) ? x & 31u : x & 3u;
    bool two = false;
    switch (mode) {
        case 0x00: endpoints<0x00>(lo, hi, e); two = true; break;
        case 0x01: endpoints<0x01>(lo, hi, e); two = true; break;
        case 0x02: endpoints<0x02>(lo, hi, e); two = true; break;
        case 0x06: endpoints<0x06>(lo, hi, e); two = true; break;
        case 0x0a: endpoints<0x0a>(lo, hi, e); two = true; break;
        case 0x0e: endpoints<0x0e>(lo, hi, e); two = true; break;
        case 0x12: endpoints<0x12>(lo, hi, e); two = true; break;
        case 0x16: endpoints<0x16>(lo, hi, e); two = true; break;
        case 0x1a: endpoints<0x1a>(lo, hi, e); two = true; break;
        case 0x1e: endpoints<0x1e>(lo, hi, e); two = true; break;
        case 0x03: endpoints<0x03>(lo, hi, e); break;
        case 0x07: endpoints<0x07>(lo, hi, e); break;
        case 0x0b: endpoints<0x0b>(lo, hi, e); break;
        case 0x0f: endpoints<0x0f>(lo, hi, e); break;
        default: break;                                       // 0x13, 0x17, 0x1b, 0x1f are reserved: every endpoint 0, rgb = 0
    }
    return two;
}
// texel t's interpolation weight (two: nonzero for two regions, a word as texel() holds it; anchor: region 1's anchor texel, 16 for none).  Indices: 3 bits from
// block bit 82 (two regions) or 4 bits from bit 65, an anchor texel one bit fewer; all in `hi`
BC6H_DEC_FN uint32_t texel_weight(uint64_t hi, uint32_t two, uint32_t anchor, uint32_t t) {
    const uint32_t ib = two ? 3u : 4u, base = two ? 18u : 1u;
    const uint32_t start = base + ib * t - (t > 0u ? 1u : 0u) - (t > anchor ? 1u : 0u);
    const uint32_t width = ib - ((t == 0u || t == anchor) ? 1u : 0u);
    const uint32_t idx = (uint32_t)(hi >> start) & ((1u << width) - 1u);
    return (uint32_t)((two ? WEIGHTS3 : idx < 8u ? WEIGHTS4_LO : WEIGHTS4_HI) >> (8u * (idx & 7u))) & 255u;
}

// ---- per texel ----
// One block ready for texel(): the unquantized endpoints (<= 0xffff each) two to a word — pair[c] = e0 | e1 << 16, pair[3 + c] =
// e2 | e3 << 16 (c: r, g, b) —, the upper 64 bits of the block (every index bit lies there) and meta = the partition pattern (bits
// 0 .. 15, texel t in bit t; 0 for one region) | anchor << 16 (16: none) | two regions << 24.  Nine words.
struct Block {
    uint32_t pair[6];
    uint32_t hi_lo, hi_hi;
    uint32_t meta;
};

// the 16 bytes of a block (bit 0 of the block = bit 0 of x) -> Block: the mode's header once, whatever texels are asked for later
BC6H_DEC_FN Block header(uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
    const uint64_t lo = x | ((uint64_t)y << 32), hi = z | ((uint64_t)w << 32);
    uint32_t e[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    const bool two = mode_endpoints(lo, hi, e);
    const uint32_t shape = (uint32_t)(hi >> 13) & 31u;        // bits 77 .. 81
    const uint32_t pattern = two ? (uint32_t)PARTITION[shape] : 0u;
    const uint32_t anchor = !two ? 16u : shape < 16u ? 15u : (uint32_t)(ANCHOR_16_31 >> (4u * (shape - 16u))) & 15u;
    Block b;
    BC6H_DEC_UNROLL
    for (uint32_t c = 0; c < 3u; c++) {
        b.pair[c] = e[c] | (e[3u + c] << 16);
        b.pair[3u + c] = e[6u + c] | (e[9u + c] << 16);
    }
    b.hi_lo = z; b.hi_hi = w;
    b.meta = pattern | (anchor << 16) | (two ? 1u << 24 : 0u);
    return b;
}

// texel t (0 .. 15, row-major: x = t & 3, y = t >> 2) of a block -> its three half codes (<= 0x7bff)
BC6H_DEC_FN void texel(const Block& b, uint32_t t, uint32_t (&half)[3]) {
    const uint64_t hi = b.hi_lo | ((uint64_t)b.hi_hi << 32);
    const uint32_t two = b.meta >> 24;
    const uint32_t anchor = (b.meta >> 16) & 31u;
    const uint32_t w = texel_weight(hi, two, anchor, t);
    const bool second = ((b.meta >> t) & 1u) != 0u;
    BC6H_DEC_UNROLL
    for (uint32_t c = 0; c < 3u; c++) {
        const uint32_t p = second ? b.pair[3u + c] : b.pair[c];
        const uint32_t v = ((p & 0xffffu) * (64u - w) + (p >> 16) * w + 32u) >> 6;      // endpoints <= 0xffff: below 2^22
        half[c] = (v * 31u) >> 6;                                                        // <= 0x7bff: finite
    }
}

// the bit pattern of the fp32 value of a half code <= 0x7bff, exactly (subnormal halves included)
BC6H_DEC_FN uint32_t half_to_f32_bits(uint32_t h) {
    const uint32_t e = h >> 10, m = h & 1023u;
    if (e != 0u) return (h << 13) + (112u << 23);
    if (m == 0u) return 0u;
    uint32_t n = 0;                                           // m * 2^-24: normalise the 10-bit mantissa
    BC6H_DEC_UNROLL
    for (uint32_t k = 0; k < 10u; k++) n += (m >> k) > 1u ? 1u : 0u;     // floor(log2(m))
    return ((103u + n) << 23) | ((m << (23u - n)) & 0x7fffffu);
}

BC6H_DEC_FN float half_to_f32(uint32_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (float)__builtin_bit_cast(_Float16, (uint16_t)h);  // one conversion, the same value
#else
    return __builtin_bit_cast(float, half_to_f32_bits(h));
#endif
}

}  // namespace bc6h_dec
