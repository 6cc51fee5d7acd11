// sun.hip — pbr_sun_light: a directional light with a shadow map, added to the HDR target after the shade, and pbr_sun_fit, the
// orthographic light camera around a world box (host only).  The rule is pinned in include/pbr_hip.h and restated in
// tests/sun_truth.py; this unit is built with -ffp-contract=off and uses IEEE divides and square roots only, so the restatement
// is bit for bit.
#include <cmath>
#include "pbr_device.hpp"
#include "pbr_internal.hpp"

using namespace pbr;

namespace {

struct SunParams {
    const uint32_t* A; const uint32_t* B; const uint32_t* C; const float* depth; const uint8_t* stencil;
    const float* map;      // NULL: no shadows
    pbr_half* hdr;         // exactly one of hdr / probe
    float* probe;
    uint32_t gb_pitch, out_pitch, map_w, map_h, map_pitch, pcf;
    uint32_t x0, y0, w, h;
    float full_w, full_h;
    float InvView[9], CameraPos[3];
    float Near, Far, near_width, near_height;
    float L[3], Lum[3], M[12], bias_const, bias_slope;
};

__device__ __forceinline__ float dot_lr(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 unit_exact(V3 v) { const float l = sqrtf(dot_lr(v, v)); return v3(v.x / l, v.y / l, v.z / l); }
__device__ __forceinline__ float lerp_t(float a, float b, float w) { return a + (b - a) * w; }

// one tap: lit outside the map, and where the receiver is not behind the stored depth (a tie is lit)
__device__ __forceinline__ float tap(const SunParams& p, int tx, int ty, float zr) {
    if ((uint32_t)tx >= p.map_w || (uint32_t)ty >= p.map_h) return 1.0f;
    return zr <= p.map[(uint32_t)ty * p.map_pitch + (uint32_t)tx] ? 1.0f : 0.0f;
}

__device__ __forceinline__ float visibility(const SunParams& p, V3 q, float NdotL) {
    if (p.map == nullptr) return 1.0f;
    const float zr = q.z - (p.bias_const + p.bias_slope * (1.0f - NdotL));
    const float su = ((q.x + 1.0f) * 0.5f) * (float)p.map_w - 0.5f;
    const float sv = ((1.0f - q.y) * 0.5f) * (float)p.map_h - 0.5f;
    if (!(q.z >= 0.0f && q.z <= 1.0f)) return 1.0f;
    if (!(su >= -2.0f && su < (float)p.map_w + 1.0f && sv >= -2.0f && sv < (float)p.map_h + 1.0f)) return 1.0f;   // NaN lands here
    const float fu = floorf(su), fv = floorf(sv);
    const float wx = su - fu, wy = sv - fv;
    const int ix = (int)fu, iy = (int)fv;   // in [-2, map + 1): exact
    if (p.pcf == 1u) {
        const float t00 = tap(p, ix, iy, zr), t10 = tap(p, ix + 1, iy, zr), t01 = tap(p, ix, iy + 1, zr), t11 = tap(p, ix + 1, iy + 1, zr);
        return lerp_t(lerp_t(t00, t10, wx), lerp_t(t01, t11, wx), wy);
    }
    // pcf 3: the 4 x 4 taps once; every tap row lerped along x into its three footprint columns, then pairs of rows along y
    float hrow[4][3];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float t0 = tap(p, ix - 1, iy - 1 + j, zr), t1 = tap(p, ix, iy - 1 + j, zr), t2 = tap(p, ix + 1, iy - 1 + j, zr),
                    t3 = tap(p, ix + 2, iy - 1 + j, zr);
        hrow[j][0] = lerp_t(t0, t1, wx); hrow[j][1] = lerp_t(t1, t2, wx); hrow[j][2] = lerp_t(t2, t3, wx);
    }
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int i = 0; i < 3; i++) s = s + lerp_t(hrow[j][i], hrow[j + 1][i], wy);
    return s * (1.0f / 9.0f);
}

// lane = pixel; a work unit is one 256-pixel piece of a tile row (one wave reads one segment per G-buffer plane), persistent grid
template <bool PROBE>
__global__ __launch_bounds__(256) void k_sun_light(const SunParams p) {
    const uint32_t upr = (p.w + 255u) >> 8, units = upr * p.h;
    const float inv255 = 1.0f / 255.0f;
    for (uint32_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t y = unit / upr, x = (unit - y * upr) * 256u + threadIdx.x;
        if (x >= p.w) continue;
        const uint32_t gi = y * p.gb_pitch + x, oi = y * p.out_pitch + x;   // host-checked: pitch * rows * 16 < 2^32
        float cr = 0.0f, cg = 0.0f, cb = 0.0f, vis = 0.0f;
        bool lit = false;
        if (p.stencil[gi] != 0) {
            const uint32_t a = p.A[gi], b = p.B[gi], c = p.C[gi];
            const float depth = p.depth[gi];
            const V3 N = unit_exact(decode_octahedron((float)(b & 255u) * inv255, (float)((b >> 8) & 255u) * inv255));
            const V3 L = v3(p.L[0], p.L[1], p.L[2]);
            const float NdotL = dot_lr(N, L);
            if (NdotL > 0.0f) {
                lit = true;
                // position and view vector: vs_main :91-121, ReconstructWorldPosition :79-83 (the GLOBAL pixel)
                const float u = ((float)(p.x0 + x) + 0.5f) / p.full_w, v = ((float)(p.y0 + y) + 0.5f) / p.full_h;
                const float cvv_x = (2.0f * u - 1.0f) * 0.5f * p.near_width, cvv_y = (1.0f - 2.0f * v) * 0.5f * p.near_height;
                const V3 cv = v3((p.InvView[0] * cvv_x + p.InvView[1] * cvv_y) + p.InvView[2] * p.Near,
                                 (p.InvView[3] * cvv_x + p.InvView[4] * cvv_y) + p.InvView[5] * p.Near,
                                 (p.InvView[6] * cvv_x + p.InvView[7] * cvv_y) + p.InvView[8] * p.Near);
                const float z_vs = view_space_depth(depth, p.Near, p.Far);
                const float zs = z_vs / p.Near;
                const V3 cam = v3(p.CameraPos[0], p.CameraPos[1], p.CameraPos[2]);
                const V3 P = v3(cam.x + cv.x * zs, cam.y + cv.y * zs, cam.z + cv.z * zs);
                const V3 V = unit_exact(cam - P);
                // brdf.hlsli:47-67
                const float roughness = (float)(c & 255u) * inv255, metallic = (float)((c >> 8) & 255u) * inv255;
                const V3 albedo = v3((float)(a & 255u) * inv255, (float)((a >> 8) & 255u) * inv255, (float)((a >> 16) & 255u) * inv255);
                const V3 H = unit_exact(L + V);
                const float NdotV = fmaxf(dot_lr(N, V), 0.0f), NdotH = fmaxf(dot_lr(N, H), 0.0f);
                const float pw = fmaxf(1.0f - NdotL, EPSILON_F);
                const float p5 = ((pw * pw) * (pw * pw)) * pw;
                const float ra = roughness * roughness;
                const float t = (NdotH * NdotH) * (ra * ra - 1.0f) + 1.0f;
                const float D = (ra * ra) / fmaxf((PI_F * t) * t, EPSILON_F);
                const float k = ((roughness + 1.0f) * (roughness + 1.0f)) * 0.125f;
                const float G = (NdotV / fmaxf(NdotV * (1.0f - k) + k, EPSILON_F)) * (NdotL / fmaxf(NdotL * (1.0f - k) + k, EPSILON_F));
                const float den = fmaxf((4.0f * NdotL) * NdotV, 0.0001f);
                auto channel = [&](float alb, float lum) {
                    const float F0 = 0.04f + (alb - 0.04f) * metallic;
                    const float F = F0 + (1.0f - F0) * p5;
                    const float Kd = (1.0f - F) * (1.0f - metallic);
                    const float brdf = (Kd * alb) * INV_PI_F + ((F * D) * G) / den;
                    return (brdf * lum) * NdotL;
                };
                cr = channel(albedo.x, p.Lum[0]); cg = channel(albedo.y, p.Lum[1]); cb = channel(albedo.z, p.Lum[2]);
                const V3 q = v3(((p.M[0] * P.x + p.M[1] * P.y) + p.M[2] * P.z) + p.M[3],
                                ((p.M[4] * P.x + p.M[5] * P.y) + p.M[6] * P.z) + p.M[7],
                                ((p.M[8] * P.x + p.M[9] * P.y) + p.M[10] * P.z) + p.M[11]);
                vis = visibility(p, q, NdotL);
            }
        }
        if constexpr (PROBE) {
            reinterpret_cast<float4*>(p.probe)[oi] = lit ? make_float4(cr * vis, cg * vis, cb * vis, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        } else {
            if (lit && vis != 0.0f) {
                H4* px = reinterpret_cast<H4*>(p.hdr) + oi;
                H4 hv = *px;
                hv.x = to_half_rn((float)hv.x + cr * vis);
                hv.y = to_half_rn((float)hv.y + cg * vis);
                hv.z = to_half_rn((float)hv.z + cb * vis);
                *px = hv;   // alpha's bits as read
            }
        }
    }
}

bool finite_all(const float* v, int n) {
    for (int i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

}  // namespace

extern "C" {

pbr_status pbr_sun_light(pbr_ctx* ctx, const pbr_sun_desc* d) {
    const char* who = "pbr_sun_light";
    if (!ctx) return PBR_ERR_INVALID;
    if (!d || !d->g || !d->tile || !d->gb || !d->sun) return refuse(ctx, who, "null pointer");
    const pbr_global& g = *d->g;
    const pbr_tile& t = *d->tile;
    const pbr_gbuffer& gb = *d->gb;
    const pbr_sun& s = *d->sun;
    if (!(gb.A && gb.B && gb.C && gb.depth && gb.stencil)) return refuse(ctx, who, "null G-buffer plane");
    if ((d->hdr != nullptr) == (d->contrib_f32 != nullptr)) return refuse(ctx, who, "exactly one of hdr / contrib_f32");
    if (!(t.w >= 1 && t.h >= 1)) return refuse(ctx, who, "empty tile");
    if (!(t.full_w >= 1 && t.full_h >= 1 && (uint64_t)t.x0 + t.w <= t.full_w && (uint64_t)t.y0 + t.h <= t.full_h))
        return refuse(ctx, who, "tile outside its frame");
    if (!(gb.pitch >= t.w && d->hdr_pitch >= t.w)) return refuse(ctx, who, "pitch < width");
    if (!((uint64_t)gb.pitch * t.h * 16u < (1ull << 32) && (uint64_t)d->hdr_pitch * t.h * 16u < (1ull << 32)))
        return refuse(ctx, who, "target too large for 32-bit plane offsets (pitch x rows x 16 bytes must stay below 4 GiB)");
    if (!(s.pcf == 1u || s.pcf == 3u)) return refuse(ctx, who, "pcf must be 1 or 3");
    if (!finite_all(s.Direction, 3) || !finite_all(s.Luminance, 3) || !finite_all(s.LightViewProj, 16) || !std::isfinite(s.bias_const) ||
        !std::isfinite(s.bias_slope))
        return refuse(ctx, who, "non-finite sun");
    const double dd = (double)s.Direction[0] * s.Direction[0] + (double)s.Direction[1] * s.Direction[1] + (double)s.Direction[2] * s.Direction[2];
    if (!(std::fabs(dd - 1.0) <= 1e-4)) return refuse(ctx, who, "Direction is not unit (|d.d - 1| <= 1e-4)");
    const float* M = s.LightViewProj;
    if (!(M[12] == 0.0f && M[13] == 0.0f && M[14] == 0.0f && M[15] == 1.0f)) return refuse(ctx, who, "LightViewProj is not affine");
    if (!(g.Near > 0.0f && g.Far > g.Near)) return refuse(ctx, who, "need 0 < Near < Far");
    float cam[16] = {g.Near, g.Far, g.Fov, g.Ratio, g.CameraPos[0], g.CameraPos[1], g.CameraPos[2]};
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) cam[7 + 3 * r + c] = g.InvView[4 * r + c];
    if (!finite_all(cam, 16)) return refuse(ctx, who, "non-finite camera (Near, Far, Fov, Ratio, CameraPos, InvView)");
    if (d->shadow_depth) {
        if (!(d->map_w >= 1 && d->map_h >= 1 && d->map_w <= PBR_RASTER_MAX_SIZE && d->map_h <= PBR_RASTER_MAX_SIZE))
            return refuse(ctx, who, "map size of 0 or above PBR_RASTER_MAX_SIZE");
        if (!(d->map_pitch >= d->map_w)) return refuse(ctx, who, "map_pitch < map_w");
        if (!((uint64_t)d->map_pitch * d->map_h * 4u < (1ull << 32))) return refuse(ctx, who, "map too large for 32-bit offsets");
    }
    if ((addr(gb.A) | addr(gb.B) | addr(gb.C) | addr(gb.depth) | addr(d->shadow_depth)) & 3u || addr(d->hdr) & 7u || addr(d->contrib_f32) & 15u)
        return refuse(ctx, who, "misaligned plane");

    SunParams p{};
    p.A = gb.A; p.B = gb.B; p.C = gb.C; p.depth = gb.depth; p.stencil = gb.stencil; p.gb_pitch = gb.pitch;
    p.map = d->shadow_depth; p.map_w = d->map_w; p.map_h = d->map_h; p.map_pitch = d->map_pitch; p.pcf = s.pcf;
    p.hdr = d->hdr; p.probe = d->contrib_f32; p.out_pitch = d->hdr_pitch;
    p.x0 = t.x0; p.y0 = t.y0; p.w = t.w; p.h = t.h; p.full_w = (float)t.full_w; p.full_h = (float)t.full_h;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) p.InvView[r * 3 + c] = g.InvView[r * 4 + c];
    for (int i = 0; i < 3; i++) { p.CameraPos[i] = g.CameraPos[i]; p.L[i] = s.Direction[i]; p.Lum[i] = s.Luminance[i]; }
    p.Near = g.Near; p.Far = g.Far;
    p.near_height = (float)(2.0 * (double)g.Near * std::tan((double)g.Fov / 2.0));   // its own, not pbr::camera_near_plane: the double-precision tan is pinned by tests/sun_truth.py
    p.near_width = p.near_height * g.Ratio;
    for (int i = 0; i < 12; i++) p.M[i] = M[i];
    p.bias_const = s.bias_const; p.bias_slope = s.bias_slope;

    const uint64_t units = (uint64_t)((t.w + 255u) >> 8) * t.h;
    const uint64_t cap = (uint64_t)(ctx->cu_count > 0 ? ctx->cu_count : 256) * 8u;
    const uint32_t blocks = (uint32_t)(units < cap ? units : cap);
    if (d->contrib_f32) hipLaunchKernelGGL(k_sun_light<true>, dim3(blocks), dim3(256), 0, ctx->stream, p);
    else hipLaunchKernelGGL(k_sun_light<false>, dim3(blocks), dim3(256), 0, ctx->stream, p);
    return launched(ctx, "k_sun_light");
}

pbr_status pbr_sun_fit(const float dir[3], const pbr_aabb* world_box, uint32_t map_w, uint32_t map_h, pbr_global* light_g,
                       float light_view_proj[16]) {
    if (!dir || !world_box || !light_g || !light_view_proj) return PBR_ERR_INVALID;
    if (!(map_w >= 3 && map_h >= 3 && map_w <= PBR_RASTER_MAX_SIZE && map_h <= PBR_RASTER_MAX_SIZE)) return PBR_ERR_INVALID;
    if (!finite_all(dir, 3) || !finite_all(world_box->min, 3) || !finite_all(world_box->max, 3)) return PBR_ERR_INVALID;
    for (int i = 0; i < 3; i++)
        if (world_box->min[i] > world_box->max[i]) return PBR_ERR_INVALID;
    const double len = std::sqrt(((double)dir[0] * dir[0] + (double)dir[1] * dir[1]) + (double)dir[2] * dir[2]);
    if (!(len > 0.0)) return PBR_ERR_INVALID;
    const double d[3] = {dir[0] / len, dir[1] / len, dir[2] / len};
    const double z[3] = {-d[0], -d[1], -d[2]};
    const double up[3] = {std::fabs(d[1]) > 0.999 ? 1.0 : 0.0, std::fabs(d[1]) > 0.999 ? 0.0 : 1.0, 0.0};
    double x[3] = {up[1] * z[2] - up[2] * z[1], up[2] * z[0] - up[0] * z[2], up[0] * z[1] - up[1] * z[0]};
    const double xl = std::sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
    for (int i = 0; i < 3; i++) x[i] = x[i] / xl;
    const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
    const double* axes[3] = {x, y, z};
    double lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        for (int corner = 0; corner < 8; corner++) {
            const double px = (corner & 1) ? world_box->max[0] : world_box->min[0];
            const double py = (corner & 2) ? world_box->max[1] : world_box->min[1];
            const double pz = (corner & 4) ? world_box->max[2] : world_box->min[2];
            const double v = (axes[a][0] * px + axes[a][1] * py) + axes[a][2] * pz;
            if (corner == 0 || v < lo[a]) lo[a] = v;
            if (corner == 0 || v > hi[a]) hi[a] = v;
        }
        if (hi[a] - lo[a] < 1e-6) {
            const double c = (lo[a] + hi[a]) * 0.5;
            lo[a] = c - 0.5e-6; hi[a] = c + 0.5e-6;
        }
    }
    const double ex = (hi[0] - lo[0]) / (double)(map_w - 2u), ey = (hi[1] - lo[1]) / (double)(map_h - 2u), ez = 0.01 * (hi[2] - lo[2]);
    const double l = lo[0] - ex, r = hi[0] + ex, b = lo[1] - ey, t = hi[1] + ey, n = lo[2] - ez, f = hi[2] + ez;

    *light_g = pbr_global{};
    float* V = light_g->View; float* IV = light_g->InvView; float* P = light_g->Projection; float* IP = light_g->InvProjection;
    for (int a = 0; a < 3; a++)
        for (int c = 0; c < 3; c++) { V[4 * a + c] = (float)axes[a][c]; IV[4 * c + a] = (float)axes[a][c]; }
    V[15] = IV[15] = 1.0f;
    P[0] = (float)(2.0 / (r - l)); P[3] = (float)(-(r + l) / (r - l));
    P[5] = (float)(2.0 / (t - b)); P[7] = (float)(-(t + b) / (t - b));
    P[10] = (float)(1.0 / (f - n)); P[11] = (float)(-n / (f - n));
    P[15] = 1.0f;
    IP[0] = (float)((r - l) / 2.0); IP[3] = (float)((r + l) / 2.0);
    IP[5] = (float)((t - b) / 2.0); IP[7] = (float)((t + b) / 2.0);
    IP[10] = (float)(f - n); IP[11] = (float)n;
    IP[15] = 1.0f;
    light_g->Resolution[0] = (float)map_w; light_g->Resolution[1] = (float)map_h;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double acc = 0.0;
            for (int k2 = 0; k2 < 4; k2++) acc = acc + (double)P[4 * i + k2] * (double)V[4 * k2 + j];
            light_view_proj[4 * i + j] = (float)acc;
        }
    return PBR_OK;
}

}  // extern "C"
