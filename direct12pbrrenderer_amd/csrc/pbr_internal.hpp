// pbr_internal.hpp — host-side context shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include <cstdio>
#include <cstdlib>
#include "../../include/pbr_hip.h"

struct pbr_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    void* scratch = nullptr;          // device scratch (SH partials, ...)
    size_t scratch_bytes = 0;
    std::string err;
    std::vector<float> host_tmp;      // host staging (prefilter sample tables)
    // pbr_prefilter_env: the sample tables of the last (size, mips, sky mips), kept on the device between calls
    void* pf_dev = nullptr;
    uint32_t pf_key[3] = {0, 0, 0};
    uint32_t pf_count[16] = {};
    float pf_wsum[16] = {};
    // RCCL (loaded lazily with dlopen so a 1-GPU run never needs librccl)
    void* rccl_lib = nullptr;
    void* comm = nullptr;             // frame communicator: halo exchange (ncclSend / ncclRecv)
    void* comm_hist = nullptr;        // ncclCommSplit of it: the histogram all-reduce (may run on the side stream)
    int world = 1;
    int rank = 0;
    // high-priority side stream of pbr_ctx_side_begin / _end / _join
    hipStream_t side_stream = nullptr, main_saved = nullptr;
    hipEvent_t ev_side_fork = nullptr, ev_side_join = nullptr;
    bool on_side = false, side_pending = false, main_was_null = false;
    std::vector<uint32_t> side_cu_mask;   // pbr_ctx_set_cu_masks: the side stream's CUs (empty: all, high priority)
    bool bloom_shader_order = false;      // pbr_ctx_set_bloom_shader_order: large 2x-up bloom levels in the shader's operation order (bit-exact)
    int cu_count = 0;                     // compute units of the device (the shade sizes its blocks by the resident-block count)
    // pbr_launch_log: the labels of the last PBR_LAUNCH_LOG launches (string literals, a ring) and how many launches there were
    const char* launch_log[PBR_LAUNCH_LOG] = {};
    uint64_t launch_count = 0;
};

namespace pbr {

inline pbr_status fail(pbr_ctx* ctx, pbr_status code, const char* what) {
    if (ctx) ctx->err = what;
    return code;
}
// a check shared by several entry points returns what is wrong (nullptr: nothing) and the caller refuses under its own name
inline pbr_status refuse(pbr_ctx* ctx, const char* who, const char* why) {
    if (ctx) ctx->err = std::string(who) + ": " + why;
    return PBR_ERR_INVALID;
}
inline pbr_status hip_fail(pbr_ctx* ctx, hipError_t e, const char* where) {
    if (ctx) {
        ctx->err = std::string(where) + ": " + hipGetErrorString(e);
    }
    return PBR_ERR_HIP;
}
// after a kernel launch; `where` is a string literal: the launch log keeps the pointer
inline pbr_status launched(pbr_ctx* ctx, const char* where) {
    ctx->launch_log[ctx->launch_count++ % PBR_LAUNCH_LOG] = where;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(ctx, e, where);
    return PBR_OK;
}

constexpr size_t SCRATCH_BYTES = 1u << 20;

// Tuning / A-B switches of the launch code.  The PRODUCT library takes every one at its built-in value and never reads the
// environment: a drop-in must not change its kernel choice on an environment variable.  A build with -DPBR_DEBUG_KNOBS
// (`make knobs` -> libpbr_hip_knobs.so; used by the tests that force a kernel choice and by the sweep scripts through
// PBR_HIP_LIB) reads PBR_<NAME> once per call site.
inline const char* knob_text(const char* name) {
#ifdef PBR_DEBUG_KNOBS
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}
inline int knob_int(const char* name, int dflt) { const char* v = knob_text(name); return v ? atoi(v) : dflt; }
inline float knob_float(const char* name, float dflt) { const char* v = knob_text(name); return v ? (float)atof(v) : dflt; }
inline bool knob_set(const char* name) { return knob_text(name) != nullptr; }

// Multi-view calls (pbr_*_views): the view count, and no byte of one view's outputs inside another view's.  range(view, k, lo, hi)
// gives the byte range [lo, hi) of output k < n_out of a view (null pointers are checked before).
inline bool views_count_ok(const pbr_view* v, uint32_t n) { return v != nullptr && n >= 1 && n <= (uint32_t)PBR_MAX_VIEWS; }
template <class F>
inline bool views_disjoint(const pbr_view* v, uint32_t n, int n_out, F range) {
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t j = i + 1; j < n; j++)
            for (int a = 0; a < n_out; a++)
                for (int b = 0; b < n_out; b++) {
                    uintptr_t a0, a1, b0, b1;
                    range(v[i], a, a0, a1);
                    range(v[j], b, b0, b1);
                    if (a0 < b1 && b0 < a1) return false;
                }
    return true;
}
inline uintptr_t addr(const void* p) { return (uintptr_t)p; }
// The camera of g as the screen-space kernels take it: the 3x3 part of InvView (row-major) and the near plane's size,
// 2 Near tan(Fov/2) high and Ratio times that wide (vs_main :94-95), in float with the host's libm.
inline void camera_near_plane(const pbr_global* g, float inv_view[9], float& near_width, float& near_height) {
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) inv_view[r * 3 + c] = g->InvView[r * 4 + c];
    near_height = 2.0f * g->Near * tanf(g->Fov / 2.0f);
    near_width = near_height * g->Ratio;
}
// the view argument of a single-view kernel instantiation: empty; placed in a padding hole of the argument block, it moves no argument
struct NoViews {};

}  // namespace pbr

#define PBR_REQUIRE(ctx, cond, msg) \
    do { if (!(cond)) return pbr::fail((ctx), PBR_ERR_INVALID, msg); } while (0)
#define PBR_CHECK(ctx, who, check) \
    do { if (const char* why__ = (check)) return pbr::refuse((ctx), (who), why__); } while (0)
#define PBR_HIP(ctx, call) \
    do { hipError_t e__ = (call); if (e__ != hipSuccess) return pbr::hip_fail((ctx), e__, #call); } while (0)
