// bc6h_decode.hip — the reference's load-time decode of a sky asset on the GPU (include/pbr_hip.h, "BC6H sky cubes"): a CubeMapResource
// holds six DXGI_FORMAT_BC6H_UF16 chains (TextureCompression.h:13-14, ResourceDef.cpp:187-219) that DirectX::Decompress expands when
// the file is read; pbr_bc6h_decode_cube expands them into the fp32 RGBA cube chain every consumer here takes (pbr_cube_f32).
//   k_bc6h_decode_cube   all faces and all levels in one launch, lane = block.  The block is one 16-byte load (a wave reads 1 KiB of
//                        consecutive blocks) kept as two 64-bit words; a switch on the mode runs that mode's header as straight-line
//                        bit-field extracts (every field position is a template constant: the four words never become an indexed
//                        array), applies the delta transform and unquantizes; the code after the switch is shared: per texel one
//                        64-bit shift of the upper word gives the index (all index bits lie there), a shift of a packed constant the
//                        weight, then three interpolations, and each texel leaves as one 16-byte store — a lane writes the block's
//                        rows as 4 x 64 bytes, lanes adjacent in x cover a contiguous run of a row.  No LDS, no cross-lane traffic.
//                        A wave runs every mode its lanes hold: random blocks are the worst case, a real sky uses few modes per
//                        neighbourhood.
// The rule is pinned in the header; tests/bc6h_ref.py restates it in numpy (held to a third-party decoder on the CPU) and the kernel
// is held to that bit for bit.
#include <cstdint>

#include "pbr_internal.hpp"
#include "pbr_device.hpp"

namespace {

constexpr uint32_t BC6H_MAX_LEVELS = 14;    // floor(log2(PBR_BC6H_MAX_SIZE)) + 1
static_assert((1u << (BC6H_MAX_LEVELS - 1)) == PBR_BC6H_MAX_SIZE, "levels of the largest cube");

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

// texel t in bit t: set = the second endpoint pair (e2 / e3)
__constant__ uint16_t PARTITION[32] = {0xcccc, 0x8888, 0xeeee, 0xecc8, 0xc880, 0xfeec, 0xfec8, 0xec80, 0xc800, 0xffec, 0xfe80,
                                       0xe800, 0xffe8, 0xff00, 0xfff0, 0xf000, 0xf710, 0x008e, 0x7100, 0x08ce, 0x008c, 0x7310,
                                       0x3100, 0x8cce, 0x088c, 0x3110, 0x6666, 0x366c, 0x17e8, 0x0ff0, 0x718e, 0x399c};
constexpr uint64_t ANCHOR_16_31 = 0x22882282f882282full;      // region 1's anchor texel of shapes 16 .. 31, a nibble each (0 .. 15: 15)
constexpr uint64_t WEIGHTS3 = 0x40372e251b120900ull;          // 0, 9, 18, 27, 37, 46, 55, 64: a byte each
constexpr uint64_t WEIGHTS4_LO = 0x1e1a15110d090400ull;       // 0, 4, 9, 13, 17, 21, 26, 30
constexpr uint64_t WEIGHTS4_HI = 0x403c37332f2b2622ull;       // 34, 38, 43, 47, 51, 55, 60, 64

// bits POS .. POS + N - 1 of the block
template <uint32_t POS, uint32_t N>
__device__ __forceinline__ uint32_t block_bits(uint64_t lo, uint64_t hi) {
    static_assert(N >= 1 && N <= 16 && POS + N <= 128, "a header field");
    uint64_t v;
    if constexpr (POS >= 64) v = hi >> (POS - 64);
    else if constexpr (POS + N <= 64) v = lo >> POS;
    else v = (lo >> POS) | (hi << (64 - POS));
    return (uint32_t)v & ((1u << N) - 1u);
}
template <uint32_t M, uint32_t S, uint32_t POS>
__device__ __forceinline__ void read_header(uint64_t lo, uint64_t hi, uint32_t (&e)[12]) {
    constexpr ModeDesc D = mode_desc(M);
    if constexpr (S < D.count) {
        constexpr Seg g = D.segs[S];
        uint32_t v = block_bits<POS, g.n>(lo, hi);
        if constexpr (g.rev != 0) v = __brev(v) >> (32u - g.n);
        e[g.field] |= v << g.lo;
        read_header<M, S + 1, POS + g.n>(lo, hi, e);
    }
}
template <uint32_t N>
__device__ __forceinline__ uint32_t unquantize(uint32_t x) {
    if constexpr (N >= 15) return x;
    else return x == 0u ? 0u : x == (1u << N) - 1u ? 0xffffu : ((x << 15) + 0x4000u) >> (N - 1u);
}
// a mode's header -> its unquantized endpoints e[3 i + c] (i: e0 .. e3, c: r, g, b); one-region modes leave e2 / e3 zero
template <uint32_t M>
__device__ __forceinline__ void endpoints(uint64_t lo, uint64_t hi, uint32_t (&e)[12]) {
    constexpr ModeDesc D = mode_desc(M);
    read_header<M, 0, (M < 2 ? 2u : 5u)>(lo, hi, e);
    constexpr uint32_t mask = (1u << D.endpoint_bits) - 1u, last = D.two ? 3u : 1u;
    if constexpr (D.transformed) {
#pragma unroll
        for (uint32_t i = 1; i <= last; i++) {
#pragma unroll
            for (uint32_t c = 0; c < 3u; c++) {
                const uint32_t sh = 32u - D.delta_bits[c];
                e[3u * i + c] = (e[c] + (uint32_t)((int32_t)(e[3u * i + c] << sh) >> sh)) & mask;
            }
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < 3u * (last + 1u); k++) e[k] = unquantize<D.endpoint_bits>(e[k]);
}

struct Bc6hCube {
    const uint4* face[6];
    uint32_t face_first[BC6H_MAX_LEVELS + 1];   // blocks of one face in front of the level; [mips] = one face's blocks
    uint32_t first_texel[BC6H_MAX_LEVELS];      // pbr_cube_mip_offset of the level
    uint32_t size, mips;
    uint32_t lanes;                             // 6 x one face's blocks
};

// lane = block; the lanes of a level are face after face, the face's blocks row-major
__global__ __launch_bounds__(256) void k_bc6h_decode_cube(Bc6hCube L, float4* __restrict__ out) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= L.lanes) return;
    uint32_t l = 0, ff = 0, ft = 0;
#pragma unroll
    for (uint32_t k = 1; k < BC6H_MAX_LEVELS; k++) {          // (static indices: the table stays in scalar registers)
        if (k < L.mips && g >= 6u * L.face_first[k]) { l = k; ff = L.face_first[k]; ft = L.first_texel[k]; }
    }
    const uint32_t s = L.size >> l, bw = max(1u, (s + 3u) >> 2), nb = bw * bw;
    const uint32_t k = g - 6u * ff, f = k / nb, r = k - f * nb, by = r / bw, bx = r - by * bw;
    const uint4* src = f == 0 ? L.face[0] : f == 1 ? L.face[1] : f == 2 ? L.face[2] : f == 3 ? L.face[3] : f == 4 ? L.face[4] : L.face[5];
    const uint4 q = src[ff + r];
    const uint64_t lo = q.x | ((uint64_t)q.y << 32), hi = q.z | ((uint64_t)q.w << 32);

    uint32_t e[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    const uint32_t mode = (q.x & 2u) ? q.x & 31u : q.x & 3u;
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

    // indices: 3 bits from block bit 82 (two regions) or 4 bits from bit 65, an anchor texel one bit fewer; all in `hi`
    const uint32_t shape = (uint32_t)(hi >> 13) & 31u;        // bits 77 .. 81
    const uint32_t pattern = two ? (uint32_t)PARTITION[shape] : 0u;
    const uint32_t anchor = !two ? 16u : shape < 16u ? 15u : (uint32_t)(ANCHOR_16_31 >> (4u * (shape - 16u))) & 15u;
    const uint32_t ib = two ? 3u : 4u, base = two ? 18u : 1u;
    float4* dst = out + ft + ((size_t)f * s + 4u * by) * s + 4u * bx;
#pragma unroll
    for (uint32_t t = 0; t < 16u; t++) {
        const uint32_t x = t & 3u, y = t >> 2;
        const uint32_t start = base + ib * t - (t > 0u ? 1u : 0u) - (t > anchor ? 1u : 0u);
        const uint32_t width = ib - ((t == 0u || t == anchor) ? 1u : 0u);
        const uint32_t idx = (uint32_t)(hi >> start) & ((1u << width) - 1u);
        const uint32_t w = (uint32_t)((two ? WEIGHTS3 : idx < 8u ? WEIGHTS4_LO : WEIGHTS4_HI) >> (8u * (idx & 7u))) & 255u;
        const bool second = (pattern >> t) & 1u;
        float c[3];
#pragma unroll
        for (uint32_t ch = 0; ch < 3u; ch++) {
            const uint32_t a = second ? e[6u + ch] : e[ch], b = second ? e[9u + ch] : e[3u + ch];
            const uint32_t v = (a * (64u - w) + b * w + 32u) >> 6;            // a, b <= 0xffff: below 2^22
            const uint16_t h = (uint16_t)((v * 31u) >> 6);                    // <= 0x7bff: finite
            c[ch] = (float)__builtin_bit_cast(_Float16, h);                   // exact, subnormal halves included
        }
        if (4u * bx + x < s && 4u * by + y < s) dst[(size_t)y * s + x] = make_float4(c[0], c[1], c[2], 1.0f);
    }
}

uint32_t max_levels(uint32_t size) {
    uint32_t n = 0;
    while (size) { n++; size >>= 1; }
    return n;
}
uint32_t level_blocks(uint32_t s) { const uint32_t b = (s + 3u) / 4u; return b ? b : 1u; }
bool chain_ok(uint32_t size, uint32_t mip_levels) {
    return size >= 4u && size <= PBR_BC6H_MAX_SIZE && (size & 3u) == 0 && mip_levels >= 1u && mip_levels <= max_levels(size);
}

}  // namespace

extern "C" {

size_t pbr_bc6h_chain_bytes(uint32_t size, uint32_t mip_levels) {
    if (!chain_ok(size, mip_levels)) return 0;
    size_t blocks = 0;
    for (uint32_t l = 0; l < mip_levels; l++) blocks += (size_t)level_blocks(size >> l) * level_blocks(size >> l);
    return 16u * blocks;
}

pbr_status pbr_bc6h_decode_cube(pbr_ctx* ctx, const void* const face_blocks[6], uint32_t size, uint32_t mip_levels, float* out_rgba) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, face_blocks && out_rgba, "pbr_bc6h_decode_cube: null pointer");
    PBR_REQUIRE(ctx, chain_ok(size, mip_levels),
                "pbr_bc6h_decode_cube: size 0, not a multiple of 4 or above PBR_BC6H_MAX_SIZE, or mip_levels 0 or above floor(log2(size)) + 1");
    PBR_REQUIRE(ctx, (pbr::addr(out_rgba) & 15u) == 0, "pbr_bc6h_decode_cube: out_rgba not 16-byte aligned");
    Bc6hCube L;
    for (int f = 0; f < 6; f++) {
        PBR_REQUIRE(ctx, face_blocks[f], "pbr_bc6h_decode_cube: null face pointer");
        PBR_REQUIRE(ctx, (pbr::addr(face_blocks[f]) & 15u) == 0, "pbr_bc6h_decode_cube: face blocks not 16-byte aligned");
        L.face[f] = static_cast<const uint4*>(face_blocks[f]);
    }
    L.size = size; L.mips = mip_levels;
    uint32_t nb = 0;                              // (the largest face chain holds 2048^2 * 4 / 3 blocks, the cube 8192^2 * 8 texels: below 2^32)
    for (uint32_t l = 0; l <= BC6H_MAX_LEVELS; l++) {
        L.face_first[l] = nb;
        if (l < BC6H_MAX_LEVELS) L.first_texel[l] = (uint32_t)pbr::cube_mip_offset(size, l < mip_levels ? l : mip_levels);
        if (l < mip_levels) nb += level_blocks(size >> l) * level_blocks(size >> l);
    }
    L.lanes = 6u * nb;
    hipLaunchKernelGGL(k_bc6h_decode_cube, dim3((L.lanes + 255u) / 256u), dim3(256), 0, ctx->stream, L, reinterpret_cast<float4*>(out_rgba));
    return pbr::launched(ctx, "k_bc6h_decode_cube");
}

}  // extern "C"
