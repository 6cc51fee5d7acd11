// DeferredPipeline.cpp — Execute bodies: bind by shader resource name, set the POD constants,
// dispatch with the reference's group counts (Engine/Source/Renderer/Pipeline/DeferredPipeline.cpp).
#include "DeferredPipeline.h"

#include <cfloat>
#include <cmath>

namespace MRendererHip {

static inline uint32 CalculateDispatchSize(uint32 texture_size, uint32 thread_group_size) {
    return (texture_size + thread_group_size - 1) / thread_group_size;
}
template <class T>
static T* As(IDeviceResource* r) {
    T* t = dynamic_cast<T*>(r);
    if (!t) throw HipException("frame-graph resource has an unexpected type");
    return t;
}

std::vector<IRenderPass*> DeferredRenderPipeline::Setup() {
    // construction order matters exactly as in the reference: BloomPass reads DeferredShadingRT's
    // description from the table, so DeferredShadingPass must exist first (DeferredPipeline.cpp:24-33)
    mPrefilterEnvMapPass = std::make_unique<PreFilterEnvMapPass>(mEnvSize);
    mPrecomputeBRDFPass = std::make_unique<PrecomputeBRDFPass>(mLutRes);
    mGBufferPass = std::make_unique<GBufferPass>(mSize);
    mDeferredShadingPass = std::make_unique<DeferredShadingPass>(mSize);
    mSkyboxPass = std::make_unique<SkyboxPass>();
    mAutoExposurePass = std::make_unique<AutoExposurePass>();
    mToneMappingPass = std::make_unique<ToneMappingPass>(mSize);
    mPresentPass = std::make_unique<PresentPass>();
    mBloomPass = std::make_unique<BloomPass>(mHaloChain);
    mClusteredPass = std::make_unique<ClusteredPass>();
    mPresentPass->SetFinalTexture(DeferredPipelineResource::ToneMappedTexture);
    mPasses = {mPrefilterEnvMapPass.get(), mPrecomputeBRDFPass.get(), mClusteredPass.get(), mGBufferPass.get(),
               mDeferredShadingPass.get(), mSkyboxPass.get(), mAutoExposurePass.get(), mToneMappingPass.get(), mBloomPass.get(), mPresentPass.get()};
    mAntiAliasing = false;
    mSunShadowPass.reset();
    mSunLightPass.reset();
    return mPasses;
}

std::vector<IRenderPass*> DeferredRenderPipeline::Compose() const {
    std::vector<IRenderPass*> passes = mPasses;
    if (mSunShadowPass) passes.insert(passes.end() - 1, mSunShadowPass.get());   // in front of Present, the list's last
    if (mSunLightPass) passes.insert(passes.end() - 1, mSunLightPass.get());
    if (mAntiAliasing) passes.insert(passes.end() - 1, mAntiAliasPass.get());
    return passes;
}

std::vector<IRenderPass*> DeferredRenderPipeline::SetSunLight(bool on, const SunSettings& sun) {
    if (mPasses.empty()) throw HipException("DeferredRenderPipeline::SetSunLight: Setup() first");
    if (mSunPending) throw HipException("DeferredRenderPipeline::SetSunLight: CommitSunLight or RollbackSunLight first");
    // everything that can refuse comes before anything is changed
    const double x = sun.Direction[0], y = sun.Direction[1], z = sun.Direction[2], len = std::sqrt((x * x + y * y) + z * z);
    if (on && (!(len > 0.0) || !std::isfinite(len))) throw HipException("SetSunLight: the direction is zero or not finite");
    // the passes the frame graph still points at stay alive (and the settings they read stay as they are) until CommitSunLight
    mOldSunShadowPass = std::move(mSunShadowPass);
    mOldSunLightPass = std::move(mSunLightPass);
    mOldSun = mSun;
    mSunPending = true;
    mBloomPass->ClearRunAfter();
    if (on) {
        const uint64_t serial = mSun.Serial + 1;
        mSun = sun;
        mSun.Serial = serial;
        mSun.Direction[0] = (float)(x / len); mSun.Direction[1] = (float)(y / len); mSun.Direction[2] = (float)(z / len);
        if (mSun.Shadows) mSunShadowPass = std::make_unique<SunShadowPass>(mGBufferPass.get(), &mSun);
        mSunLightPass = std::make_unique<SunLightPass>(&mSun, mSun.Shadows);
        mBloomPass->RunAfter(mSunLightPass.get());
    }
    return Compose();
}

void DeferredRenderPipeline::CommitSunLight() {
    mOldSunShadowPass.reset();
    mOldSunLightPass.reset();
    mSunPending = false;
}

std::vector<IRenderPass*> DeferredRenderPipeline::RollbackSunLight() {
    if (mSunPending) {
        mSunShadowPass = std::move(mOldSunShadowPass);
        mSunLightPass = std::move(mOldSunLightPass);
        mSun = mOldSun;
        mBloomPass->ClearRunAfter();
        if (mSunLightPass) mBloomPass->RunAfter(mSunLightPass.get());
        mSunPending = false;
    }
    return Compose();
}

std::vector<IRenderPass*> DeferredRenderPipeline::SetAntiAliasing(bool on) {
    if (mPasses.empty()) throw HipException("DeferredRenderPipeline::SetAntiAliasing: Setup() first");
    if (on && !mAntiAliasPass) mAntiAliasPass = std::make_unique<AntiAliasPass>();
    mAntiAliasing = on;
    mPresentPass->SetFinalTexture(on ? DeferredPipelineResource::AntiAliasedTexture : DeferredPipelineResource::ToneMappedTexture);
    return Compose();
}

// ----------------------------------------------------------------------------------- IBL precompute
PreFilterEnvMapPass::PreFilterEnvMapPass(uint32 size) : mSize(size), mReady(false) {
    if ((size >> (PreFilterEnvMapMipsLevel - 1)) < 1)   // the coarsest mip must still hold a texel
        throw HipException("PreFilterEnvMapPass: size too small for 5 mips");
    mPrefilterEnvMap = std::make_shared<DeviceTexture2DArray>(size, PreFilterEnvMapMipsLevel, ETextureFormat_R16G16B16A16_FLOAT);
    WritePersistentResource(DeferredPipelineResource::PrefilterEnvMap, mPrefilterEnvMap.get());
}

void PreFilterEnvMapPass::Execute(FGContext* context) {   // DeferredPipeline.cpp:77-115
    if (mReady) return;
    mReady = true;
    SkyBox* sky = context->Scene->GetSkyBox();
    if (!sky) return;
    PIXScope(context->CommandList, "Precompute PrefilterEnvMap Pass");
    // a sky resident as BC6H blocks is decoded into a cube that lives for this pass only (once per sky: the fence below is no frame cost)
    DeviceTexture* source = sky->Resource();
    std::unique_ptr<DeviceTexture2DArray> decoded;
    if (auto* blocks = dynamic_cast<DeviceBc6hCube*>(source)) {
        decoded = std::make_unique<DeviceTexture2DArray>(blocks->Size(), blocks->MipLevels(), ETextureFormat_R32G32B32A32_FLOAT);
        context->CommandList->DecodeBc6hCube(blocks, decoded.get());
        source = decoded.get();
    }
    struct Release {      // the commands that read `decoded` are done before it is freed, on every way out
        HipCommandList* cl; bool wait;
        ~Release() { if (wait) { try { cl->WaitIdle(); } catch (...) {} } }
    } release{context->CommandList, decoded != nullptr};
    if (context->CommandList->FusedPasses()) {   // the five dispatches below as one call (same roughness ladder: mip / 4)
        auto* cube = dynamic_cast<DeviceTexture2DArray*>(source);
        if (!cube) throw HipException("PreFilterEnvMapPass: the sky box is not a cube texture");
        context->CommandList->PrefilterEnv(cube, mPrefilterEnvMap.get());
        return;
    }
    for (uint32 i = 0; i < PreFilterEnvMapMipsLevel; i++) {
        ShadingState& st = mShadingState[i];
        st.SetShader("env_map_gen.hlsl", true);
        st.SetRWTextureArray("PrefilterEnvMap", mPrefilterEnvMap.get());
        st.SetTexture("SkyBox", source);
        st.SetConstantBuffer(PreFilterEnvMapConstant{(float)i / (float)(PreFilterEnvMapMipsLevel - 1), i, mSize});
    }
    for (uint32 i = 0; i < PreFilterEnvMapMipsLevel; i++) {
        const uint32 mip_size = mSize >> i;
        const uint32 groups = (mip_size + DispatchGroupSize - 1) / DispatchGroupSize;
        context->CommandList->Dispatch(&mShadingState[i], groups, groups, 6);
    }
}

PrecomputeBRDFPass::PrecomputeBRDFPass(uint32 res) : mRes(res), mReady(false) {
    mPrecomputeBRDF = std::make_shared<DeviceTexture2D>(res, res, 1, ETextureFormat_R16G16_FLOAT);
    WritePersistentResource(DeferredPipelineResource::PrecomputeBRDF, mPrecomputeBRDF.get());
    mShadingState.SetShader("precompute_brdf.hlsl", true);
    mShadingState.SetRWTexture("PrecomputeBRDF", mPrecomputeBRDF.get());
}

void PrecomputeBRDFPass::Execute(FGContext* context) {   // :117-136
    if (mReady) return;
    PIXScope(context->CommandList, "Precompute BRDF Pass");
    mReady = true;
    constexpr uint32 ThreadGroupSize = 8;
    mShadingState.SetConstantBuffer(PrecomputeBRDFConstant{mRes});
    context->CommandList->Dispatch(&mShadingState, (mRes + ThreadGroupSize - 1) / ThreadGroupSize, (mRes + ThreadGroupSize - 1) / ThreadGroupSize, 1);
}

// ----------------------------------------------------------------------------------- G-buffer (input)
GBufferPass::GBufferPass(RenderSize s) {
    WriteTransientTexture(DeferredPipelineResource::GBufferA, s.Width, s.Height, 1, ETextureFormat_R8G8B8A8_UNORM);
    WriteTransientTexture(DeferredPipelineResource::GBufferB, s.Width, s.Height, 1, ETextureFormat_R8G8B8A8_UNORM);
    WriteTransientTexture(DeferredPipelineResource::GBufferC, s.Width, s.Height, 1, ETextureFormat_R8G8B8A8_UNORM);
    WriteTransientTexture(DeferredPipelineResource::DepthStencil, s.Width, s.Height, 1, ETextureFormat_DepthStencil, ETexture2DFlag_AllowDepthStencil);
    mShadingState.SetShader("gbuffer.hlsl", false);
}

void GBufferPass::UploadMeshes(FGContext* context, MeshSource& meshes, uint32 w, uint32 h) {
    if (context->CommandList->FramesInFlight() > 1) context->CommandList->WaitIdle();   // earlier frames still read the buffers
    uint64_t tris = 0;
    for (const pbr_draw& d : meshes.Draws) tris += d.index_count / 3u;
    if (tris == 0 || tris > PBR_RASTER_MAX_TRIANGLES) throw HipException("GBufferPass: the draws hold no triangles, or more than PBR_RASTER_MAX_TRIANGLES");
    auto upload = [](std::unique_ptr<DeviceStructuredBuffer>& buf, const void* data, size_t bytes, uint32 stride) {
        if (bytes > 0xffffffffu) throw HipException("GBufferPass: mesh buffer larger than 4 GiB");
        buf = std::make_unique<DeviceStructuredBuffer>((uint32)bytes, stride);
        buf->Commit(data, bytes);
    };
    upload(mVertices, meshes.Vertices.data(), meshes.Vertices.size() * sizeof(pbr_vertex), sizeof(pbr_vertex));
    upload(mIndices, meshes.Indices.data(), meshes.Indices.size() * sizeof(uint32_t), sizeof(uint32_t));
    upload(mDraws, meshes.Draws.data(), meshes.Draws.size() * sizeof(pbr_draw), sizeof(pbr_draw));
    mMaxTriangles = (uint32)tris;
    mMaps.reset();
    mTextures.clear();
    mTextureTable.clear();
    if (meshes.Textured()) {
        upload(mMaps, meshes.Maps.data(), meshes.Maps.size() * sizeof(pbr_draw_maps), sizeof(pbr_draw_maps));
        for (const TextureChain& t : meshes.Textures) {   // one allocation per chain: BC1 blocks land 8-byte aligned
            mTextures.emplace_back();
            upload(mTextures.back(), t.Texels.data(), t.Texels.size(), 1);
            mTextureTable.push_back(pbr_texture2d{mTextures.back()->DevicePtr(), t.Width, t.Height, t.MipLevels, t.Format});
        }
    }
    const size_t scratch = meshes.Textured() ? pbr_gbuffer_raster_textured_scratch_bytes(w, h, mMaxTriangles)
                                             : pbr_gbuffer_raster_scratch_bytes(w, h, mMaxTriangles);
    if (scratch > 0xffffffffu) throw HipException("GBufferPass: raster scratch larger than 4 GiB");
    mRasterScratch = std::make_unique<DeviceStructuredBuffer>((uint32)scratch, 4);
    mBounds.reset();
    mCullStats.reset();
    if (meshes.Cull) {   // the AABB the reference's mesh files carry, made from the buffers just uploaded
        mBounds = std::make_unique<DeviceStructuredBuffer>((uint32)(meshes.Draws.size() * sizeof(pbr_aabb)), (uint32)sizeof(pbr_aabb));
        mCullStats = std::make_unique<DeviceStructuredBuffer>((uint32)sizeof(pbr_cull_stats), (uint32)sizeof(pbr_cull_stats));
        const pbr_cull_stats zero{0, 0, 0, 0};
        mCullStats->Commit(&zero, sizeof(zero));
        context->CommandList->DrawBounds((const pbr_vertex*)mVertices->DevicePtr(), (uint32)meshes.Vertices.size(),
                                         (const uint32_t*)mIndices->DevicePtr(), (uint32)meshes.Indices.size(),
                                         (const pbr_draw*)mDraws->DevicePtr(), (uint32)meshes.Draws.size(), (pbr_aabb*)mBounds->DevicePtr());
    }
    meshes.Dirty = false;
    mUploads++;
}

void GBufferPass::CullingStatus(uint32_t out[4]) const {
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!mCullStats) return;
    pbr_cull_stats st;
    ThrowIfFailed(hipMemcpy(&st, mCullStats->DevicePtr(), sizeof(st), hipMemcpyDeviceToHost), "read culling status");
    out[0] = st.draws_drawn; out[1] = st.draws_culled; out[2] = st.triangles_drawn; out[3] = st.triangles_culled;
}

pbr_raster_desc GBufferPass::RasterInputs() const {
    pbr_raster_desc d{};
    if (!mRasterScratch) return d;
    auto count = [](const DeviceStructuredBuffer& b) { return b.Size() / b.Stride(); };
    d.vertices = (const pbr_vertex*)mVertices->DevicePtr(); d.n_vertices = count(*mVertices);
    d.indices = (const uint32_t*)mIndices->DevicePtr(); d.n_indices = count(*mIndices);
    d.draws = (const pbr_draw*)mDraws->DevicePtr(); d.n_draws = count(*mDraws);
    d.max_triangles = mMaxTriangles;
    d.scratch = mRasterScratch->DevicePtr(); d.scratch_bytes = mRasterScratch->Size();
    if (mMaps) {
        d.maps = (const pbr_draw_maps*)mMaps->DevicePtr();
        d.textures = mTextureTable.empty() ? nullptr : mTextureTable.data(); d.n_textures = (uint32)mTextureTable.size();
    }
    if (mBounds) {   // Scene::CullModel + mCullingStatus (:141-150), on the device
        d.bounds = (const pbr_aabb*)mBounds->DevicePtr();
        d.stats = (pbr_cull_stats*)mCullStats->DevicePtr();
    }
    return d;
}

void GBufferPass::Execute(FGContext* context) {
    PIXScope(context->CommandList, "Gbuffer Pass");
    MeshSource& meshes = context->Scene->Meshes();
    if (!meshes.Empty()) {   // DrawModel per draw (DeferredPipeline.cpp:138-185): gbuffer.hlsl + DefaultOpaque, in draw order
        auto* a = As<DeviceTexture2D>(GetTransientResource(context, DeferredPipelineResource::GBufferA));
        auto* b = As<DeviceTexture2D>(GetTransientResource(context, DeferredPipelineResource::GBufferB));
        auto* c = As<DeviceTexture2D>(GetTransientResource(context, DeferredPipelineResource::GBufferC));
        auto* ds = As<DeviceTexture2D>(GetTransientResource(context, DeferredPipelineResource::DepthStencil));
        if (meshes.Dirty || !mRasterScratch) UploadMeshes(context, meshes, a->Width(), a->Height());
        context->CommandList->RasterGBuffer(&mShadingState, RasterInputs(), a, b, c, ds);
        return;
    }
    GBufferSource& src = context->Scene->GBuffer();
    if (!src.Dirty) return;   // the planes a rasterizer would have left in device memory are still there
    src.Dirty = false;
    if (context->CommandList->FramesInFlight() > 1) context->CommandList->WaitIdle();   // earlier frames still read the planes
    auto* a = As<DeviceTexture2D>(GetTransientResource(context, DeferredPipelineResource::GBufferA));
    if (src.Width != a->Width() || src.Height != a->Height()) throw HipException("GBufferPass: G-buffer source size != render size");
    const size_t n = (size_t)src.Width * src.Height;
    auto* b = As<DeviceTexture2D>(GetTransientResource(context, DeferredPipelineResource::GBufferB));
    auto* c = As<DeviceTexture2D>(GetTransientResource(context, DeferredPipelineResource::GBufferC));
    auto* ds = As<DeviceTexture2D>(GetTransientResource(context, DeferredPipelineResource::DepthStencil));
    if (src.HasMaterials()) {   // gbuffer.hlsl::ps_main on the rasterizer's per-pixel attributes
        if (!mMaterialPlanes || mMaterialPlanes->Size() != n * 48)
            mMaterialPlanes = std::make_unique<DeviceStructuredBuffer>((uint32)(n * 48), 16);
        float* m = (float*)mMaterialPlanes->DevicePtr();
        ThrowIfFailed(hipMemcpy(m, src.M0.data(), n * 16, hipMemcpyHostToDevice), "upload material plane 0");
        ThrowIfFailed(hipMemcpy(m + 4 * n, src.M1.data(), n * 16, hipMemcpyHostToDevice), "upload material plane 1");
        ThrowIfFailed(hipMemcpy(m + 8 * n, src.M2.data(), n * 16, hipMemcpyHostToDevice), "upload material plane 2");
        context->CommandList->EncodeGBuffer(&mShadingState, m, m + 4 * n, m + 8 * n, a, b, c);
    } else {
        ThrowIfFailed(hipMemcpy(a->DevicePtr(), src.A.data(), n * 4, hipMemcpyHostToDevice), "upload GBufferA");
        ThrowIfFailed(hipMemcpy(b->DevicePtr(), src.B.data(), n * 4, hipMemcpyHostToDevice), "upload GBufferB");
        ThrowIfFailed(hipMemcpy(c->DevicePtr(), src.C.data(), n * 4, hipMemcpyHostToDevice), "upload GBufferC");
    }
    ThrowIfFailed(hipMemcpy(ds->DepthPlane(), src.Depth.data(), n * 4, hipMemcpyHostToDevice), "upload depth");
    ThrowIfFailed(hipMemcpy(ds->StencilPlane(), src.Stencil.data(), n, hipMemcpyHostToDevice), "upload stencil");
}

SkyboxPass::SkyboxPass() {   // DeferredPipeline.cpp:46-57
    mShadingState.SetShader("skybox.hlsl", false);
    WriteResource(DeferredPipelineResource::DeferredShadingRT);
    WriteResource(DeferredPipelineResource::DepthStencil);
}
void SkyboxPass::Execute(FGContext* context) {   // DeferredPipeline.cpp:59-75
    SkyBox* sky_box = context->Scene->GetSkyBox();
    if (!sky_box) return;
    PIXScope(context->CommandList, "Skybox Pass");
    mShadingState.SetTexture("SkyBox", sky_box->Resource());
    context->CommandList->DrawMesh(&mShadingState);   // sky sphere, depth test on / write off
}

// ----------------------------------------------------------------------------------- deferred shading
DeferredShadingPass::DeferredShadingPass(RenderSize s) {   // DeferredPipeline.h:157-182
    ReadResource(DeferredPipelineResource::GBufferA);
    ReadResource(DeferredPipelineResource::GBufferB);
    ReadResource(DeferredPipelineResource::GBufferC);
    ReadResource(DeferredPipelineResource::DepthStencil);
    ReadResource(DeferredPipelineResource::PrefilterEnvMap);
    ReadResource(DeferredPipelineResource::PrecomputeBRDF);
    ReadResource(DeferredPipelineResource::PointLights);
    ReadResource(DeferredPipelineResource::FrustumCluster);
    WriteTransientTexture(DeferredPipelineResource::DeferredShadingRT, s.Width, s.Height, 1, ETextureFormat_R16G16B16A16_FLOAT,
                          (ETexture2DFlag)(ETexture2DFlag_AllowRenderTarget | ETexture2DFlag_AllowUnorderedAccess));
    WriteResource(DeferredPipelineResource::DepthStencil);   // stencil test only
    mShadingState.SetShader("deferred_shading.hlsl", false);
}

void DeferredShadingPass::Execute(FGContext* context) {   // DeferredPipeline.cpp:187-206
    PIXScope(context->CommandList, "Deferred Shading");
    auto tex = [&](FGResourceId id) { return As<DeviceTexture>(GetTransientResource(context, id)); };
    mShadingState.SetTexture("GBufferA", tex(DeferredPipelineResource::GBufferA));
    mShadingState.SetTexture("GBufferB", tex(DeferredPipelineResource::GBufferB));
    mShadingState.SetTexture("GBufferC", tex(DeferredPipelineResource::GBufferC));
    mShadingState.SetTexture("PrefilterEnvMap", tex(DeferredPipelineResource::PrefilterEnvMap));
    mShadingState.SetTexture("PrecomputeBRDF", tex(DeferredPipelineResource::PrecomputeBRDF));
    mShadingState.SetTexture("DepthStencil", tex(DeferredPipelineResource::DepthStencil));
    mShadingState.SetStructuredBuffer("Clusters", As<DeviceStructuredBuffer>(GetTransientResource(context, DeferredPipelineResource::FrustumCluster)));
    mShadingState.SetStructuredBuffer("PointLights", As<DeviceStructuredBuffer>(GetTransientResource(context, DeferredPipelineResource::PointLights)));
    context->CommandList->SetStencilRef(0);
    context->CommandList->DrawScreen(&mShadingState);
}

// ----------------------------------------------------------------------------------- clustered lights
ClusteredPass::ClusteredPass() {
    WriteTransientBuffer(DeferredPipelineResource::FrustumCluster, ClusterSizeX * ClusterSizeY * ClusterSizeZ * (uint32)sizeof(pbr_cluster), sizeof(pbr_cluster));
    WriteTransientBuffer(DeferredPipelineResource::PointLights, MaxSceneLights * (uint32)sizeof(pbr_light), sizeof(pbr_light));
    mClusteredCompute.SetShader("clustered_compute.hlsl", true);
    mClusteredCulling.SetShader("clustered_culling.hlsl", true);
}

void ClusteredPass::Execute(FGContext* context) {   // DeferredPipeline.cpp:208-258
    PIXScope(context->CommandList, "Clustered Pass");
    auto* sw_cluster = As<DeviceStructuredBuffer>(GetTransientResource(context, DeferredPipelineResource::FrustumCluster));
    auto* sw_point_light = As<DeviceStructuredBuffer>(GetTransientResource(context, DeferredPipelineResource::PointLights));
    mClusteredCompute.SetRWStructuredBuffer("Clusters", sw_cluster);
    mClusteredCulling.SetRWStructuredBuffer("Clusters", sw_cluster);
    mClusteredCulling.SetRWStructuredBuffer("PointLights", sw_point_light);
    if (context->Scene->GetLightCount() > (uint32)MaxSceneLights) throw HipException("ClusteredPass: more than MaxSceneLights lights");
    std::vector<pbr_light>& lights = mLights;
    lights.assign(MaxSceneLights, pbr_light{});
    // frustum culling point lights (DeferredPipeline.cpp:224-241): membership and buffer order come from the octree walk
    const int i = FillLightBuffer(context->Scene, context->Camera, lights.data(), MaxSceneLights);
    mClusteredCompute.SetConstantBuffer(ClusteredShaderConstant{i});
    mClusteredCulling.SetConstantBuffer(ClusteredShaderConstant{i});
    // the reference re-uploads the buffer every frame through its upload ring; here the device copy is rewritten only when
    // the culled list changed (a static camera and scene: never again) — and then only once no earlier frame that reads
    // it can still be in flight (throughput mode keeps several)
    if (i != mCommittedCount || mCommitted.size() != lights.size() || std::memcmp(mCommitted.data(), lights.data(), (size_t)i * sizeof(pbr_light)) != 0) {
        if (context->CommandList->FramesInFlight() > 1) context->CommandList->WaitIdle();
        sw_point_light->Commit(lights.data(), lights.size() * sizeof(pbr_light));
        mCommitted = lights;
        mCommittedCount = i;
    }
    if (context->CommandList->FusedPasses()) {
        context->CommandList->Clustered(sw_cluster, sw_point_light, i);
        return;
    }
    context->CommandList->Dispatch(&mClusteredCompute, 1, 1, 1);
    context->CommandList->Dispatch(&mClusteredCulling, 1, 1, 1);
}

// ----------------------------------------------------------------------------------- auto exposure
AutoExposurePass::AutoExposurePass() : mAvarageLuminanceInitialized(false) {
    ReadResource(DeferredPipelineResource::DeferredShadingRT);
    WriteTransientBuffer(DeferredPipelineResource::LuminanceHistogram, HistogramBinSize * (uint32)sizeof(uint32), sizeof(uint32));
    WriteTransientBuffer(DeferredPipelineResource::AverageLuminance, 1 * (uint32)sizeof(float), sizeof(float));
    mLuminanceHistogramCompute.SetShader("hdr_luminance_histogram.hlsl", true);
    mAvarageLuminanceCompute.SetShader("hdr_average_histogram.hlsl", true);
}

void AutoExposurePass::Execute(FGContext* context) {   // DeferredPipeline.cpp:260-318
    PIXScope(context->CommandList, "Auto Exposure Pass");
    auto* input_tex = As<DeviceTexture2D>(GetTransientResource(context, DeferredPipelineResource::DeferredShadingRT));
    auto* histogram = As<DeviceStructuredBuffer>(GetTransientResource(context, DeferredPipelineResource::LuminanceHistogram));
    auto* avg_luminance = As<DeviceStructuredBuffer>(GetTransientResource(context, DeferredPipelineResource::AverageLuminance));
    if (!mAvarageLuminanceInitialized) {
        mAvarageLuminanceInitialized = true;
        if (context->CommandList->FramesInFlight() > 1) context->CommandList->WaitIdle();
        avg_luminance->Commit(&mInitialLuminance, sizeof(float));
    }
    {
    PIXScope(context->CommandList, "Luminance Histogram Pass");
    mLuminanceHistogramCompute.SetRWStructuredBuffer("LuminanceHistogram", histogram);
    mLuminanceHistogramCompute.SetTexture("LuminanceTexture", input_tex);
    // multi-GPU: a device counts the interior of its tile only; one GPU: the whole texture, as the reference
    const HipCommandList::Rect& in = context->CommandList->Interior();
    const uint32 hw = in.w ? in.w : input_tex->Width(), hh = in.w ? in.h : input_tex->Height();
    mLuminanceHistogramCompute.SetConstantBuffer(LuminanceHistogramConstant{hw, hh, MinLogLuminance, InvLogLuminanceRange});
    context->CommandList->Dispatch(&mLuminanceHistogramCompute, CalculateDispatchSize(hw, HistogramComputeThreadGroupSize),
                                   CalculateDispatchSize(hh, HistogramComputeThreadGroupSize), 1);
    }
    PIXScope(context->CommandList, "Average Luminance Pass");
    mAvarageLuminanceCompute.SetRWStructuredBuffer("LuminanceHistogram", histogram);
    mAvarageLuminanceCompute.SetRWStructuredBuffer("AverageLuminance", avg_luminance);
    const uint32 pixels = mFullFramePixels ? mFullFramePixels : input_tex->Width() * input_tex->Height();
    mAvarageLuminanceCompute.SetConstantBuffer(AverageLuminanceConstant{pixels, MinLogLuminance, LogLuminanceRange});
    context->CommandList->Dispatch(&mAvarageLuminanceCompute, 1, 1, 1);
}

// ----------------------------------------------------------------------------------- tone mapping
ToneMappingPass::ToneMappingPass(RenderSize s) {
    ReadResource(DeferredPipelineResource::DeferredShadingRT);
    ReadResource(DeferredPipelineResource::AverageLuminance);
    WriteTransientTexture(DeferredPipelineResource::ToneMappedTexture, s.Width, s.Height, 1, ETextureFormat_R8G8B8A8_UNORM);
    mToneMappingRender.SetShader("hdr_tone_mapping.hlsl", false);
}

void ToneMappingPass::Execute(FGContext* context) {   // DeferredPipeline.cpp:320-336
    PIXScope(context->CommandList, "Tone Mapping Pass");
    auto* input_tex = As<DeviceTexture2D>(GetTransientResource(context, DeferredPipelineResource::DeferredShadingRT));
    auto* avg_luminance = As<DeviceStructuredBuffer>(GetTransientResource(context, DeferredPipelineResource::AverageLuminance));
    mToneMappingRender.SetRWStructuredBuffer("AverageLuminance", avg_luminance);
    mToneMappingRender.SetTexture("LuminanceTexture", input_tex);
    context->CommandList->DrawScreen(&mToneMappingRender);
}

// ----------------------------------------------------------------------------------- anti-aliasing (not in the reference)
AntiAliasPass::AntiAliasPass() {
    ReadResource(DeferredPipelineResource::ToneMappedTexture);
    // declared to the frame graph by FrameGraph::Recompile (AntiAliasPass::Target), not through the process-wide description table
    WriteResource(DeferredPipelineResource::AntiAliasedTexture);
    mAntiAliasRender.SetShader(Shader, false);
}

void AntiAliasPass::Execute(FGContext* context) {
    PIXScope(context->CommandList, "Anti-Aliasing Pass");
    auto* input_tex = As<DeviceTexture2D>(GetTransientResource(context, DeferredPipelineResource::ToneMappedTexture));
    mAntiAliasRender.SetTexture("InputTexture", input_tex);
    context->CommandList->DrawScreen(&mAntiAliasRender);
}

// ----------------------------------------------------------------------------------- sun light (not in the reference)
SunShadowPass::SunShadowPass(const GBufferPass* gbuffer, SunSettings* sun) : mGBuffer(gbuffer), mSun(sun) {
    // declared to the frame graph by FrameGraph::Recompile (SunShadowPass::Target), not through the process-wide description table
    WriteResource(DeferredPipelineResource::SunShadowDepth);
    RunAfter(gbuffer);   // GBufferPass uploads the meshes this pass rasterizes
    mShadingState.SetShader("gbuffer.hlsl", false);
}

bool SunShadowPass::WorldBox(const MeshSource& meshes, pbr_aabb* out) {
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    bool any = false;
    const size_t n_idx = meshes.Indices.size(), n_vtx = meshes.Vertices.size();
    for (const pbr_draw& d : meshes.Draws) {
        if (d.index_count < 3 || (uint64_t)d.first_index + d.index_count > n_idx) continue;
        float mn[3], mx[3];
        bool valid = false;
        for (uint32 t = 0; t < d.index_count / 3u; t++) {
            int64_t vi[3];
            bool ok = true;
            for (int k = 0; k < 3; k++) {
                vi[k] = (int64_t)meshes.Indices[d.first_index + 3u * t + k] + d.base_vertex;
                ok = ok && vi[k] >= 0 && vi[k] < (int64_t)n_vtx;
            }
            if (!ok) continue;
            for (int k = 0; k < 3; k++)
                for (int c = 0; c < 3; c++) {
                    const float p = meshes.Vertices[(size_t)vi[k]].position[c];
                    if (p != p) continue;
                    if (!valid) { for (int q = 0; q < 3; q++) { mn[q] = FLT_MAX; mx[q] = -FLT_MAX; } valid = true; }
                    if (p < mn[c]) mn[c] = p;
                    if (p > mx[c]) mx[c] = p;
                }
        }
        if (!valid || mn[0] > mx[0] || mn[1] > mx[1] || mn[2] > mx[2]) continue;
        for (int corner = 0; corner < 8; corner++) {
            const double x = (corner & 1) ? mx[0] : mn[0], y = (corner & 2) ? mx[1] : mn[1], z = (corner & 4) ? mx[2] : mn[2];
            for (int r = 0; r < 3; r++) {
                const float* m = d.Model + 4 * r;
                const double w = (((double)m[0] * x + (double)m[1] * y) + (double)m[2] * z) + (double)m[3];
                lo[r] = any ? std::min(lo[r], w) : w;
                hi[r] = any ? std::max(hi[r], w) : w;
            }
            any = true;
        }
    }
    if (!any) return false;
    for (int r = 0; r < 3; r++) {
        out->min[r] = std::nextafterf((float)lo[r], -INFINITY);
        out->max[r] = std::nextafterf((float)hi[r], INFINITY);
    }
    return true;
}

void SunShadowPass::Execute(FGContext* context) {
    MeshSource& meshes = context->Scene->Meshes();
    if (meshes.Empty()) throw HipException("SunShadowPass: a shadowed sun needs meshes (pbrh_set_meshes); set the sun without shadows for uploaded planes");
    if (mUploadsSeen == mGBuffer->Uploads() && mSerialSeen == mSun->Serial) return;   // the map on the device is this scene's under this sun
    PIXScope(context->CommandList, "Sun Shadow Pass");
    auto* target = As<DeviceTexture2D>(GetTransientResource(context, DeferredPipelineResource::SunShadowDepth));
    const uint32 n = target->Width();
    if (context->CommandList->FramesInFlight() > 1) context->CommandList->WaitIdle();   // earlier frames still read the map
    pbr_aabb box;
    if (!WorldBox(meshes, &box)) throw HipException("SunShadowPass: the meshes hold no valid triangle to fit the light's camera around");
    pbr_global light_g;
    if (pbr_sun_fit(mSun->Direction, &box, n, n, &light_g, mSun->LightViewProj) != PBR_OK) throw HipException("SunShadowPass: pbr_sun_fit refused the box or the map size");
    pbr_raster_desc d = mGBuffer->RasterInputs();   // the unculled constant-material raster of the same buffers
    if (mSun->DepthOnly) {
        // one dispatch either way: the depth plane alone, from the same buffers, on the depth raster's smaller scratch
        const size_t scratch = pbr_depth_raster_scratch_bytes(n, n, d.max_triangles);
        if (scratch > 0xffffffffu) throw HipException("SunShadowPass: shadow raster scratch larger than 4 GiB");
        mPlanes.reset();
        if (!mRasterScratch || mRasterScratch->Size() != scratch) mRasterScratch = std::make_unique<DeviceStructuredBuffer>((uint32)scratch, 4);
        pbr_depth_raster_desc dd{};
        dd.vertices = d.vertices; dd.indices = d.indices; dd.draws = d.draws;
        dd.n_vertices = d.n_vertices; dd.n_indices = d.n_indices; dd.n_draws = d.n_draws; dd.max_triangles = d.max_triangles;
        dd.scratch = mRasterScratch->DevicePtr(); dd.scratch_bytes = mRasterScratch->Size();
        context->CommandList->RasterShadowDepth(&mShadingState, &light_g, dd, target);
        mUploadsSeen = mGBuffer->Uploads();
        mSerialSeen = mSun->Serial;
        return;
    }
    d.maps = nullptr; d.textures = nullptr; d.n_textures = 0; d.bounds = nullptr; d.stats = nullptr;
    const size_t plane = (size_t)n * n * 4, scratch = pbr_gbuffer_raster_scratch_bytes(n, n, d.max_triangles);
    if (3 * plane > 0xffffffffu || scratch > 0xffffffffu) throw HipException("SunShadowPass: shadow raster buffers larger than 4 GiB");
    if (!mPlanes || mPlanes->Size() != 3 * plane) mPlanes = std::make_unique<DeviceStructuredBuffer>((uint32)(3 * plane), 4);
    if (!mRasterScratch || mRasterScratch->Size() != scratch) mRasterScratch = std::make_unique<DeviceStructuredBuffer>((uint32)scratch, 4);
    uint32_t* p = (uint32_t*)mPlanes->DevicePtr();
    d.scratch = mRasterScratch->DevicePtr(); d.scratch_bytes = mRasterScratch->Size();
    context->CommandList->RasterShadowMap(&mShadingState, &light_g, d, p, p + (size_t)n * n, p + 2 * (size_t)n * n, target);
    mUploadsSeen = mGBuffer->Uploads();
    mSerialSeen = mSun->Serial;
}

SunLightPass::SunLightPass(SunSettings* sun, bool shadows) : mSun(sun), mShadows(shadows) {
    ReadResource(DeferredPipelineResource::GBufferA);
    ReadResource(DeferredPipelineResource::GBufferB);
    ReadResource(DeferredPipelineResource::GBufferC);
    // an input that DeferredShading and the sky resolve write: this pass runs after both (and after GBuffer)
    ReadResource(DeferredPipelineResource::DepthStencil);
    if (shadows) ReadResource(DeferredPipelineResource::SunShadowDepth);
    // read-modify-write, declared as a write only: a read would put the pass behind Bloom, the target's last writer.  Bloom, which
    // declares no reads, is held behind this pass by an order edge (DeferredRenderPipeline::SetSunLight)
    WriteResource(DeferredPipelineResource::DeferredShadingRT);
    mShadingState.SetShader(Shader, false);
}

void SunLightPass::Execute(FGContext* context) {
    PIXScope(context->CommandList, "Sun Light Pass");
    auto tex = [&](FGResourceId id) { return As<DeviceTexture>(GetTransientResource(context, id)); };
    mShadingState.SetTexture("GBufferA", tex(DeferredPipelineResource::GBufferA));
    mShadingState.SetTexture("GBufferB", tex(DeferredPipelineResource::GBufferB));
    mShadingState.SetTexture("GBufferC", tex(DeferredPipelineResource::GBufferC));
    mShadingState.SetTexture("DepthStencil", tex(DeferredPipelineResource::DepthStencil));
    pbr_sun sun{};
    for (int k = 0; k < 3; k++) { sun.Direction[k] = mSun->Direction[k]; sun.Luminance[k] = mSun->Luminance[k]; }
    for (int k = 0; k < 16; k++) sun.LightViewProj[k] = mShadows ? mSun->LightViewProj[k] : (k % 5 == 0 ? 1.0f : 0.0f);
    sun.bias_const = mSun->BiasConst; sun.bias_slope = mSun->BiasSlope; sun.pcf = mSun->Pcf;
    mShadingState.SetConstantBuffer(sun);
    context->CommandList->SunLight(&mShadingState, mShadows ? As<DeviceTexture2D>(GetTransientResource(context, DeferredPipelineResource::SunShadowDepth)) : nullptr);
}

// ----------------------------------------------------------------------------------- bloom
BloomPass::BloomPass(RenderSize halo_chain) : mHalo(halo_chain.Width != 0) {   // DeferredPipeline.cpp:338-374
    const FGTransientTextureDescription& d = FGResourceDescriptionTable::Instance()->GetTransientTexture(DeferredPipelineResource::DeferredShadingRT);
    const uint32 cw = mHalo ? halo_chain.Width : d.Width, ch = mHalo ? halo_chain.Height : d.Height;
    if ((cw >> (MipmapLevel - 1)) == 0 || (ch >> (MipmapLevel - 1)) == 0) throw HipException("BloomPass: render size too small for the mip chain");
    WriteTransientTexture(DeferredPipelineResource::BloomMipchain, cw, ch, MipmapLevel, d.Format, ETexture2DFlag_AllowUnorderedAccess);
    WriteTransientTexture(DeferredPipelineResource::BloomTempTexture, cw, ch, MipmapLevel, d.Format, ETexture2DFlag_AllowUnorderedAccess);
    WriteResource(DeferredPipelineResource::DeferredShadingRT);
    mPrefilter.SetShader("bloom_prefilter.hlsl", true);
    mUpsampleBlurH.SetShader("blur_horizontal.hlsl", true);
    mUpsampleBlurV.SetShader("blur_vertical.hlsl", true);
    mUpsampleMerge.SetShader("bloom_merge.hlsl", true);
    for (auto& s : mDownsampleH) s.SetShader("blur_horizontal.hlsl", true);
    for (auto& s : mDownsampleV) s.SetShader("blur_vertical.hlsl", true);
    for (auto& s : mUpsampleH) s.SetShader("bloom_upsample_add.hlsl", true);
    for (auto& s : mUpsampleV) s.SetShader("blur_vertical.hlsl", true);
}

void BloomPass::Execute(FGContext* context) {   // DeferredPipeline.cpp:400-570, 16 dispatches
    PIXScope(context->CommandList, "Bloom Pass");
    auto* original_tex = As<DeviceTexture2D>(GetTransientResource(context, DeferredPipelineResource::DeferredShadingRT));
    auto* mip_chain = As<DeviceTexture2D>(GetTransientResource(context, DeferredPipelineResource::BloomMipchain));
    auto* temp_tex = As<DeviceTexture2D>(GetTransientResource(context, DeferredPipelineResource::BloomTempTexture));
    HipCommandList* cmd = context->CommandList;
    auto texel = [](uint32 w, uint32 h) { return Vector2{1.0f / (float)w, 1.0f / (float)h}; };
    if (mHalo) {
        // multi-GPU halo mode (SURVEY 8e option 2; not in the reference): the pyramid runs on the tile's extended rectangle,
        // whose level 1 outside the interior arrives from the neighbouring devices — prefilter the interior, exchange,
        // levels 1..4 + merge.  Bit-identical to the sixteen dispatches below on the whole frame in the interior.
        cmd->BloomHalo(original_tex, mip_chain, temp_tex, 1.0f, 0.5f);
        return;
    }
    if (cmd->FusedPasses()) {   // the sixteen dispatches below as one call: same HDR result
        cmd->Bloom(original_tex, mip_chain, temp_tex, 1.0f, 0.5f);
        return;
    }

    {
    PIXScope(cmd, "Bloom Prefilter");
    mPrefilter.SetConstantBuffer(BloomPrefilterConstant{texel(original_tex->Width() >> 1, original_tex->Height() >> 1), 1.0f, 0.5f});
    mPrefilter.SetTexture("InputTexture", original_tex);
    mPrefilter.SetRWTexture("OutputTexture", mip_chain, 1);
    cmd->Dispatch(&mPrefilter, CalculateDispatchSize(temp_tex->Width(), 16), CalculateDispatchSize(temp_tex->Height(), 16), 1);   // full-res grid (Q9)
    }
    {
    PIXScope(cmd, "Bloom Downsample");
    for (uint32 i = 0; i < BloomStep; i++) {   // downsample
        const uint32 upper = i + 1;
        const uint32 lw = temp_tex->Width() >> (upper + 1), lh = temp_tex->Height() >> (upper + 1);
        mDownsampleH[i].SetConstantBuffer(BlurConstant{texel(lw, lh)});
        mDownsampleH[i].SetTexture("InputTexture", mip_chain, upper);
        mDownsampleH[i].SetRWTexture("OutputTexture", temp_tex, upper + 1);
        { PIXScope(cmd, "Blur Horizontal"); cmd->Dispatch(&mDownsampleH[i], CalculateDispatchSize(lw, 256), CalculateDispatchSize(lh, 1), 1); }
        mDownsampleV[i].SetConstantBuffer(BlurConstant{texel(lw, lh)});
        mDownsampleV[i].SetTexture("InputTexture", temp_tex, i + 2);
        mDownsampleV[i].SetRWTexture("OutputTexture", mip_chain, i + 2);
        { PIXScope(cmd, "Blur Vertical"); cmd->Dispatch(&mDownsampleV[i], CalculateDispatchSize(lw, 1), CalculateDispatchSize(lh, 256), 1); }
    }
    }
    {
    PIXScope(cmd, "Bloom Upsample");
    for (int i = (int)BloomStep - 1; i >= 0; i--) {   // upsample: V(H(t1) + H(t2))
        const uint32 upper = (uint32)i + 1;
        const uint32 uw = temp_tex->Width() >> upper, uh = temp_tex->Height() >> upper;
        mUpsampleH[i].SetConstantBuffer(BlurConstant{texel(uw, uh)});
        mUpsampleH[i].SetTexture("UpperLevel", mip_chain, upper);
        mUpsampleH[i].SetTexture("LowerLevel", mip_chain, upper + 1);
        mUpsampleH[i].SetRWTexture("OutputTexture", temp_tex, i + 1);
        { PIXScope(cmd, "Upsample Horizontal Add"); cmd->Dispatch(&mUpsampleH[i], CalculateDispatchSize(uw, 256), CalculateDispatchSize(uh, 1), 1); }
        mUpsampleV[i].SetConstantBuffer(BlurConstant{texel(uw, uh)});
        mUpsampleV[i].SetTexture("InputTexture", temp_tex, upper);
        mUpsampleV[i].SetRWTexture("OutputTexture", mip_chain, upper);
        { PIXScope(cmd, "Blur Vertical"); cmd->Dispatch(&mUpsampleV[i], CalculateDispatchSize(uw, 1), CalculateDispatchSize(uh, 256), 1); }
    }
    }
    PIXScope(cmd, "Upsample Merge");
    const uint32 w = temp_tex->Width(), h = temp_tex->Height();   // merge
    mUpsampleBlurH.SetConstantBuffer(BlurConstant{texel(w, h)});
    mUpsampleBlurH.SetTexture("InputTexture", mip_chain, 1);
    mUpsampleBlurH.SetRWTexture("OutputTexture", temp_tex, 0);
    { PIXScope(cmd, "Blur Horizontal"); cmd->Dispatch(&mUpsampleBlurH, CalculateDispatchSize(w, 256), CalculateDispatchSize(h, 1), 1); }
    mUpsampleBlurV.SetConstantBuffer(BlurConstant{texel(w, h)});
    mUpsampleBlurV.SetTexture("InputTexture", temp_tex, 0);
    mUpsampleBlurV.SetRWTexture("OutputTexture", mip_chain, 0);
    { PIXScope(cmd, "Blur Vertical"); cmd->Dispatch(&mUpsampleBlurV, CalculateDispatchSize(w, 1), CalculateDispatchSize(h, 256), 1); }
    mUpsampleMerge.SetTexture("InputTexture", mip_chain, 0);
    mUpsampleMerge.SetRWTexture("OutputTexture", original_tex, 0);
    { PIXScope(cmd, "Merge"); cmd->Dispatch(&mUpsampleMerge, CalculateDispatchSize(original_tex->Width(), 16), CalculateDispatchSize(original_tex->Height(), 16), 1); }
}

}  // namespace MRendererHip
