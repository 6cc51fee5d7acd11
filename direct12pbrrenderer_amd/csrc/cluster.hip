// cluster.hip — clustered-light set-up: frustum-cluster AABBs and per-cluster light lists.
//
// Reference: clustered_compute.hlsl:8-42 and clustered_culling.hlsl:11-41, both dispatched as ONE
// 24x16-thread group whose threads walk 8 z-slices x NumLight lights serially
// (DeferredPipeline.cpp:253-256).  On MI355X that shape is pure latency (one CU, 384 serial
// chains), so the cull is re-cut: one 64-lane wave per cluster tests 64 lights per step and
// compacts the hits with a ballot + prefix popcount, which keeps the reference's
// "first 32 hits in ascending light index" order exactly.
#include "pbr_internal.hpp"
#include "pbr_device.hpp"
#include <type_traits>

using namespace pbr;

struct ClusterParams {
    float Near, Far, Ratio, Fov;
    float View[12];   // rows 0..2 of the row-major view matrix
};

__device__ __forceinline__ int cluster_index3(int x, int y, int z) {   // clustered.hlsli:40-43
    return z + x * PBR_CLUSTER_Z + y * PBR_CLUSTER_X * PBR_CLUSTER_Z;
}

// view-space AABB of cluster t (clustered_compute.hlsl:8-42)
__device__ __forceinline__ void cluster_bounds(const ClusterParams& p, int t, float mn[3], float mx[3]) {
    const int z = t % PBR_CLUSTER_Z, tx = (t / PBR_CLUSTER_Z) % PBR_CLUSTER_X, ty = t / (PBR_CLUSTER_Z * PBR_CLUSTER_X);
    const float htan = tanf(p.Fov / 2.0f);
    const float znear = p.Near * powf(p.Far / p.Near, (float)z / (float)PBR_CLUSTER_Z);
    const float zfar = p.Near * powf(p.Far / p.Near, (float)(z + 1) / (float)PBR_CLUSTER_Z);
    const float minx = 2.0f * (float)tx / (float)PBR_CLUSTER_X - 1.0f, miny = 2.0f * (float)ty / (float)PBR_CLUSTER_Y - 1.0f;
    const float maxx = 2.0f * (float)(tx + 1) / (float)PBR_CLUSTER_X - 1.0f, maxy = 2.0f * (float)(ty + 1) / (float)PBR_CLUSTER_Y - 1.0f;
    // zplane_intersection: ray = (ndc.x*Ratio*tan, ndc.y*tan, 1)*Near; return ray * (view_z / ray.z)
    auto zplane = [&](float nx, float ny, float vz) {
        V3 ray = v3(nx * p.Ratio * htan, ny * htan, 1.0f) * p.Near;
        float tt = vz / ray.z;
        return ray * tt;
    };
    V3 min_near = zplane(minx, miny, znear), min_far = zplane(minx, miny, zfar);
    V3 max_near = zplane(maxx, maxy, znear), max_far = zplane(maxx, maxy, zfar);
    mn[0] = fminf(min_near.x, min_far.x); mn[1] = fminf(min_near.y, min_far.y); mn[2] = fminf(min_near.z, min_far.z);
    mx[0] = fmaxf(max_near.x, max_far.x); mx[1] = fmaxf(max_near.y, max_far.y); mx[2] = fmaxf(max_near.z, max_far.z);
}

// grid 12 x block 256: one thread per cluster (3 072); cluster t sits at index t (cluster_index3 is the same order)
__global__ __launch_bounds__(256) void k_cluster_build(ClusterParams p, pbr_cluster* __restrict__ clusters) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= PBR_NUM_CLUSTERS) return;
    float mn[3], mx[3];
    cluster_bounds(p, t, mn, mx);
    pbr_cluster* c = clusters + t;
    c->MinBound[0] = mn[0]; c->MinBound[1] = mn[1]; c->MinBound[2] = mn[2];
    c->MaxBound[0] = mx[0]; c->MaxBound[1] = mx[1]; c->MaxBound[2] = mx[2];
    c->NumLights = 0;
}

// The sphere/AABB test feeds an integer result (the light list), so it is evaluated with the
// exact operation sequence of the shader, un-contracted (no FMA) and with IEEE sqrt.
__device__ __forceinline__ bool light_hits(const ClusterParams& p, const pbr_light& l, const float* mn, const float* mx) {
#pragma clang fp contract(off)
    const float px = ((p.View[0] * l.Position[0] + p.View[1] * l.Position[1]) + p.View[2] * l.Position[2]) + p.View[3];
    const float py = ((p.View[4] * l.Position[0] + p.View[5] * l.Position[1]) + p.View[6] * l.Position[2]) + p.View[7];
    const float pz = ((p.View[8] * l.Position[0] + p.View[9] * l.Position[1]) + p.View[10] * l.Position[2]) + p.View[11];
    const float radius = l.Radius * 1.814f * sqrtf(l.Intensity);   // Q19: HLSL constant 1.814
    const float dx = px - fminf(fmaxf(px, mn[0]), mx[0]);
    const float dy = py - fminf(fmaxf(py, mn[1]), mx[1]);
    const float dz = pz - fminf(fmaxf(pz, mn[2]), mx[2]);
    return (dx * dx + dy * dy) + dz * dz < radius * radius;
}

// pbr_clustered_views: the cull with a view dimension — grid (3072/4, views), each view's parameters by value in ClusterViews
struct ClusterView {
    ClusterParams p;
    const pbr_light* lights;
    int n;
    pbr_cluster* clusters;
};
struct ClusterViews { ClusterView v[PBR_MAX_VIEWS]; };
static_assert(sizeof(ClusterViews) <= 4096 - 256, "k_cluster_cull<.., ClusterViews>: kernel arguments over 4 KiB");

// One wave culls cluster ci.  TABLES: it also writes the cluster's list in the shade's staged format into `staged` (34 dwords: padded
// count, 0, 32 entries of 4 * light index, 4 * n — the null light — from the count on), every dword of it, with plain vector stores.
template <bool BUILD, bool TABLES>
__device__ __forceinline__ void cull_cluster(const ClusterParams& p, const pbr_light* __restrict__ lights, int n, pbr_cluster* __restrict__ clusters,
                                             int ci, int lane, uint32_t* __restrict__ staged) {
    pbr_cluster* c = clusters + ci;
    float mn[3], mx[3];
    int count = 0;
    if (BUILD) {
        cluster_bounds(p, ci, mn, mx);
        if (lane < 3) { c->MinBound[lane] = mn[lane]; c->MaxBound[lane] = mx[lane]; }
    } else {
        mn[0] = c->MinBound[0]; mn[1] = c->MinBound[1]; mn[2] = c->MinBound[2];
        mx[0] = c->MaxBound[0]; mx[1] = c->MaxBound[1]; mx[2] = c->MaxBound[2];
        count = c->NumLights;   // continues a partially filled list like the reference loop condition
        count = min(max(count, 0), PBR_MAX_LIGHTS_PER_CLUSTER);
    }
    for (int base = 0; base < n && count < PBR_MAX_LIGHTS_PER_CLUSTER; base += 64) {   // wave-uniform loop
        const int i = base + lane;
        bool hit = false;
        if (i < n) hit = light_hits(p, lights[i], mn, mx);
        const unsigned long long mask = __ballot(hit);
        const int pos = count + __popcll(mask & ((1ull << lane) - 1ull));
        if (hit && pos < PBR_MAX_LIGHTS_PER_CLUSTER) {
            c->LightIndex[pos] = i;
            if (TABLES) staged[2 + pos] = 4u * (uint32_t)i;
        }
        count = min(count + __popcll(mask), PBR_MAX_LIGHTS_PER_CLUSTER);
    }
    if (lane == 0) c->NumLights = count;
    if (TABLES) {
        static_assert(PBR_MAX_LIGHTS_PER_CLUSTER == STAGED_LIST_DWORDS - 2, "staged list: one entry per list slot");
        if (lane >= count && lane < PBR_MAX_LIGHTS_PER_CLUSTER) staged[2 + lane] = 4u * (uint32_t)n;
        if (lane == 32) staged[0] = (uint32_t)staged_list_padded(count);
        if (lane == 33) staged[1] = 0u;
    }
}

// grid 3072/4 x block 256 (4 waves, one cluster per wave).  BUILD: both dispatches of ClusteredPass::Execute in one
// launch — the wave computes its cluster's bounds itself (every lane the same values) instead of reading them back.
// VS = ClusterViews: view blockIdx.y of `vs` instead of (p_, lights_, n_, clusters_); NoViews (an empty argument): the single-view kernel.
template <bool BUILD, class VS = NoViews>
__global__ __launch_bounds__(256) void k_cluster_cull(ClusterParams p_, const pbr_light* __restrict__ lights_, int n_, VS vs,
                                                        pbr_cluster* __restrict__ clusters_) {
    constexpr bool MV = !std::is_same_v<VS, NoViews>;
    const ClusterView* view = nullptr;
    if constexpr (MV) view = &vs.v[blockIdx.y];
    const ClusterParams& p = MV ? view->p : p_;
    const pbr_light* __restrict__ lights = MV ? view->lights : lights_;
    const int n = MV ? view->n : n_;
    pbr_cluster* __restrict__ clusters = MV ? view->clusters : clusters_;
    const int lane = threadIdx.x & 63;
    const int ci = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ci >= PBR_NUM_CLUSTERS) return;   // wave-uniform
    cull_cluster<BUILD, false>(p, lights, n, clusters, ci, lane, nullptr);
}

// pbr_clustered_tables: k_cluster_cull<true> whose waves also write their cluster's staged list, and ONE more block (the grid's
// last) that writes the frame half's header and light planes — a block of its own, because a cull wave leaves its light loop at 32 hits and
// does not see every light.  The planes and the two q_safe bits are the expressions of k_deferred_shade's prologue.
__global__ __launch_bounds__(256) void k_cluster_cull_tables(ClusterParams p, const pbr_light* __restrict__ lights, int n,
                                                               pbr_cluster* __restrict__ clusters, uint32_t* __restrict__ tables) {
    if (blockIdx.x < PBR_NUM_CLUSTERS / 4) {
        const int ci = blockIdx.x * 4 + (threadIdx.x >> 6);
        cull_cluster<true, true>(p, lights, n, clusters, ci, threadIdx.x & 63, tables + PBR_TABLES_LISTS + ci * STAGED_LIST_DWORDS);
        return;
    }
    const int stride = shade_light_stride(n);
    float* planes = reinterpret_cast<float*>(tables + PBR_TABLES_PLANES);
    int my_safe = 1, my_same = 1;
    const float att0 = n > 0 ? lights[0].C0 : 1.0f, att1 = n > 0 ? lights[0].C1 : 0.0f, att2 = n > 0 ? lights[0].C2 : 0.0f;
    for (int i = threadIdx.x; i < stride; i += 256) {
        float v[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (i < n) {
            const pbr_light l = lights[i];
            my_safe &= (l.C0 >= EPSILON_F) & (l.C1 >= 0.0f) & (l.C2 >= 0.0f);
            my_same &= (l.C0 == att0) & (l.C1 == att1) & (l.C2 == att2);
            v[0] = l.Position[0]; v[1] = l.Position[1]; v[2] = l.Position[2];
            v[3] = l.Color[0] * l.Intensity; v[4] = l.Color[1] * l.Intensity; v[5] = l.Color[2] * l.Intensity;
            v[6] = l.C0; v[7] = l.C1; v[8] = l.C2;
        } else if (i == n) {   // the null light: pads odd lists; black, so its pair lane contributes exactly 0
            v[0] = v[1] = v[2] = 1.0e15f;
            v[6] = 1.0f;
        }
#pragma unroll
        for (int k = 0; k < 9; k++) planes[k * stride + i] = v[k];
    }
    for (uint32_t d = 9u * (uint32_t)stride + threadIdx.x; d < PBR_TABLES_LISTS - PBR_TABLES_PLANES; d += 256u) planes[d] = 0.0f;   // the image is deterministic
    const int q_safe = (__syncthreads_and(my_safe) != 0 ? 1 : 0) | (__syncthreads_and(my_same) != 0 ? 2 : 0);
    if (threadIdx.x < 4) tables[PBR_TABLES_HEADER + threadIdx.x] = threadIdx.x == 0 ? (uint32_t)q_safe : threadIdx.x == 1 ? (uint32_t)n : threadIdx.x == 2 ? (uint32_t)stride : 0u;
}

static ClusterParams make_params(const pbr_global* g) {
    ClusterParams p;
    p.Near = g->Near; p.Far = g->Far; p.Ratio = g->Ratio; p.Fov = g->Fov;
    for (int i = 0; i < 12; i++) p.View[i] = g->View[i];
    return p;
}

// the cull's arguments (nullptr: usable; the caller refuses under its own name).  build: k_cluster_cull<true>, which also makes the
// cluster boxes from g's Near / Far (pbr_cluster_cull continues from the boxes pbr_cluster_build made)
static const char* cull_args_bad(const pbr_global* g, bool build, const pbr_light* lights, int n) {
    if (build && !(g->Near > 0.0f && g->Far > g->Near)) return "need 0 < Near < Far";
    // ClusteredPass::Execute asserts GetLightCount() <= MaxSceneLights (DeferredPipeline.cpp:222)
    if (!(n >= 0 && n <= PBR_MAX_SCENE_LIGHTS)) return "light count out of [0, 1024]";
    if (!(n == 0 || lights != nullptr)) return "null lights";
    return nullptr;
}

extern "C" {

pbr_status pbr_cluster_build(pbr_ctx* ctx, const pbr_global* g, pbr_cluster* clusters) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, g && clusters, "pbr_cluster_build: null pointer");
    PBR_REQUIRE(ctx, g->Near > 0.0f && g->Far > g->Near, "pbr_cluster_build: need 0 < Near < Far");
    hipLaunchKernelGGL(k_cluster_build, dim3(PBR_NUM_CLUSTERS / 256), dim3(256), 0, ctx->stream, make_params(g), clusters);
    return launched(ctx, "k_cluster_build");
}

pbr_status pbr_cluster_cull(pbr_ctx* ctx, const pbr_global* g, const pbr_light* lights, int n, pbr_cluster* clusters) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, g && clusters, "pbr_cluster_cull: null pointer");
    PBR_CHECK(ctx, "pbr_cluster_cull", cull_args_bad(g, false, lights, n));
    if (n == 0) return PBR_OK;
    hipLaunchKernelGGL(k_cluster_cull<false>, dim3(PBR_NUM_CLUSTERS / 4), dim3(256), 0, ctx->stream, make_params(g), lights, n, NoViews{}, clusters);
    return launched(ctx, "k_cluster_cull");
}

pbr_status pbr_clustered(pbr_ctx* ctx, const pbr_global* g, const pbr_light* lights, int n, pbr_cluster* clusters) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, g && clusters, "pbr_clustered: null pointer");
    PBR_CHECK(ctx, "pbr_clustered", cull_args_bad(g, true, lights, n));
    hipLaunchKernelGGL(k_cluster_cull<true>, dim3(PBR_NUM_CLUSTERS / 4), dim3(256), 0, ctx->stream, make_params(g), lights, n, NoViews{}, clusters);
    return launched(ctx, "k_cluster_cull<build>");
}

size_t pbr_shade_tables_bytes(uint32_t w, uint32_t h) { return ((size_t)PBR_TABLES_GEOM + 2u * (size_t)w + 2u * (size_t)h) * 4u; }

pbr_status pbr_clustered_tables(pbr_ctx* ctx, const pbr_global* g, const pbr_light* lights, int n, pbr_cluster* clusters, pbr_shade_tables* tables) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, g && clusters && tables, "pbr_clustered_tables: null pointer");
    PBR_CHECK(ctx, "pbr_clustered_tables", cull_args_bad(g, true, lights, n));
    PBR_REQUIRE(ctx, tables->dev && ((uintptr_t)tables->dev & 15u) == 0 && tables->bytes >= (uint64_t)PBR_TABLES_GEOM * 4u,
                "pbr_clustered_tables: the tables buffer must be 16-byte aligned and hold pbr_shade_tables_bytes()");
    tables->built &= ~PBR_TABLES_BUILT_FRAME;
    hipLaunchKernelGGL(k_cluster_cull_tables, dim3(PBR_NUM_CLUSTERS / 4 + 1), dim3(256), 0, ctx->stream, make_params(g), lights, n, clusters, (uint32_t*)tables->dev);
    const pbr_status r = launched(ctx, "k_cluster_cull_tables");
    if (r == PBR_OK) { tables->built |= PBR_TABLES_BUILT_FRAME; tables->num_lights = n; tables->list_pad = 2u * SHADE_WALK_TRIPS; }
    return r;
}

pbr_status pbr_clustered_views(pbr_ctx* ctx, const pbr_view* views, uint32_t n) {
    if (!ctx) return PBR_ERR_INVALID;
    PBR_REQUIRE(ctx, views_count_ok(views, n), "pbr_clustered_views: need 1 .. PBR_MAX_VIEWS views");
    ClusterViews vs{};
    for (uint32_t i = 0; i < n; i++) {
        const pbr_view& v = views[i];
        PBR_REQUIRE(ctx, v.clusters, "pbr_clustered_views: null clusters");
        PBR_CHECK(ctx, "pbr_clustered_views", cull_args_bad(&v.g, true, v.lights, v.num_lights));
        vs.v[i] = ClusterView{make_params(&v.g), v.lights, v.num_lights, v.clusters};
    }
    PBR_REQUIRE(ctx, views_disjoint(views, n, 1, [](const pbr_view& v, int, uintptr_t& lo, uintptr_t& hi) {
                    lo = addr(v.clusters); hi = lo + (size_t)PBR_NUM_CLUSTERS * sizeof(pbr_cluster); }),
                "pbr_clustered_views: two views share a cluster buffer");
    hipLaunchKernelGGL((k_cluster_cull<true, ClusterViews>), dim3(PBR_NUM_CLUSTERS / 4, n), dim3(256), 0, ctx->stream,
                       ClusterParams{}, (const pbr_light*)nullptr, 0, vs, (pbr_cluster*)nullptr);
    return launched(ctx, "k_cluster_cull<views>");
}

}  // extern "C"
