// DeferredPipeline.h — the deferred pipeline's pass classes over the HIP kernels.
//
// Same classes, resource names, constants and declared reads/writes as
// Engine/Include/Renderer/Pipeline/DeferredPipeline.h (line references per class); Execute bodies
// in DeferredPipeline.cpp bind by the reference's shader resource names and dispatch with the
// reference's thread-group counts.  GBufferPass / SkyboxPass are raster passes: GBufferPass rasterizes the
// scene's constant-material meshes (pbr_gbuffer_raster) or, without meshes, uploads either the encoded
// G-buffer planes or a rasterizer's per-pixel material attributes and encodes them with gbuffer.hlsl's
// pixel-shader math; SkyboxPass resolves the sky on the pixels geometry left uncovered.
#pragma once
#include "FrameGraph.h"
#include "Scene.h"
#include "ShaderConstants.h"

namespace MRendererHip {

struct DeferredPipelineResource {   // DeferredPipeline.h:9-32
    inline static FGResourceId PrefilterEnvMap = FGResourceIDs::Instance()->NameToID("PrefilterEnvMap");
    inline static FGResourceId PrecomputeBRDF = FGResourceIDs::Instance()->NameToID("PrecomputeBRDF");
    inline static FGResourceId GBufferA = FGResourceIDs::Instance()->NameToID("GBufferA");
    inline static FGResourceId GBufferB = FGResourceIDs::Instance()->NameToID("GBufferB");
    inline static FGResourceId GBufferC = FGResourceIDs::Instance()->NameToID("GBufferC");
    inline static FGResourceId DepthStencil = FGResourceIDs::Instance()->NameToID("GBufferDepthStencil");
    inline static FGResourceId DeferredShadingRT = FGResourceIDs::Instance()->NameToID("DeferredShadingRT");
    inline static FGResourceId BloomMipchain = FGResourceIDs::Instance()->NameToID("BloomMipchain");
    inline static FGResourceId BloomTempTexture = FGResourceIDs::Instance()->NameToID("BloomTempTexture");
    inline static FGResourceId ToneMappedTexture = FGResourceIDs::Instance()->NameToID("ToneMappedTexture");
    inline static FGResourceId FrustumCluster = FGResourceIDs::Instance()->NameToID("FrustumCluster");
    inline static FGResourceId PointLights = FGResourceIDs::Instance()->NameToID("ClusteredLights");
    inline static FGResourceId LuminanceHistogram = FGResourceIDs::Instance()->NameToID("LuminanceHistogram");
    inline static FGResourceId AverageLuminance = FGResourceIDs::Instance()->NameToID("AverageLuminance");
    // not in the reference: the target of AntiAliasPass, declared (and allocated) only while anti-aliasing is on
    inline static FGResourceId AntiAliasedTexture = FGResourceIDs::Instance()->NameToID("AntiAliasedTexture");
    // not in the reference: the sun's shadow map, the depth-stencil target of SunShadowPass; declared only while a shadowed sun is set
    inline static FGResourceId SunShadowDepth = FGResourceIDs::Instance()->NameToID("SunShadowDepth");
};

// render size (GD3D12Device->Width()/Height() in the reference; App.h:77-78 defaults 1440x960)
struct RenderSize { uint32 Width, Height; };

class PreFilterEnvMapPass : public ComputePass {   // DeferredPipeline.h:35-70
public:
    static constexpr uint32 PreFilterEnvMapSize = 512;
    static constexpr uint32 PreFilterEnvMapMipsLevel = 5;
    static constexpr uint32 DispatchGroupSize = 8;
    explicit PreFilterEnvMapPass(uint32 size = PreFilterEnvMapSize);
    const char* Name() const override { return "PreFilterEnvMap"; }
    void Execute(FGContext* context) override;
    void Invalidate() { mReady = false; }
protected:
    uint32 mSize;
    std::array<ShadingState, PreFilterEnvMapMipsLevel> mShadingState;
    std::shared_ptr<DeviceTexture2DArray> mPrefilterEnvMap;
    bool mReady;
};

class PrecomputeBRDFPass : public ComputePass {   // :72-99
public:
    static constexpr uint32 TextureResolution = 512;
    explicit PrecomputeBRDFPass(uint32 res = TextureResolution);
    const char* Name() const override { return "PrecomputeBRDF"; }
    void Execute(FGContext* context) override;
protected:
    uint32 mRes;
    ShadingState mShadingState;
    std::shared_ptr<DeviceTexture2D> mPrecomputeBRDF;
    bool mReady;
};

class GBufferPass : public GraphicsPass {   // :101-137 (meshes: pbr_gbuffer_raster; uploaded planes: pbr_gbuffer_encode)
public:
    explicit GBufferPass(RenderSize s);
    const char* Name() const override { return "GBuffer"; }
    void Execute(FGContext* context) override;
    // mCullingStatus (DeferredPipeline.h:96-100) of the last Execute with model culling on, read back from the device here (the
    // caller has drained the command list): NumDrawCall, NumCulled, triangles drawn, triangles culled; zeros without culling
    void CullingStatus(uint32_t out[4]) const;
    // the input half of a pbr_raster_desc from the device copies of the scene's meshes (all null before the first upload): geometry,
    // counts, maps and table, bounds and stats, scratch.  For Execute and for SunShadowPass (which runs after this pass, clears the
    // map and cull fields and puts in its own scratch); Uploads() counts UploadMeshes calls
    pbr_raster_desc RasterInputs() const;
    uint64_t Uploads() const { return mUploads; }
protected:
    uint64_t mUploads = 0;
    void UploadMeshes(FGContext* context, MeshSource& meshes, uint32 w, uint32 h);
    ShadingState mShadingState;
    std::unique_ptr<DeviceStructuredBuffer> mMaterialPlanes;   // device copy of GBufferSource::M0..M2
    // device copies of MeshSource and the raster's scratch (sized for the render target and the draws' triangles)
    std::unique_ptr<DeviceStructuredBuffer> mVertices, mIndices, mDraws, mRasterScratch;
    // textured draws: the maps, the texel chains and their descriptors (device pointers into mTextures)
    std::unique_ptr<DeviceStructuredBuffer> mMaps;
    std::vector<std::unique_ptr<DeviceStructuredBuffer>> mTextures;
    std::vector<pbr_texture2d> mTextureTable;
    uint32 mMaxTriangles = 0;
    // model culling: the draws' local boxes (pbr_draw_bounds at upload) and the device pbr_cull_stats every Execute rewrites
    std::unique_ptr<DeviceStructuredBuffer> mBounds, mCullStats;
};

class DeferredShadingPass : public GraphicsPass {   // :139-190
public:
    explicit DeferredShadingPass(RenderSize s);
    const char* Name() const override { return "DeferredShading"; }
protected:
    void Execute(FGContext* context) override;
    ShadingState mShadingState;
};

class SkyboxPass : public GraphicsPass {   // :192-206, DeferredPipeline.cpp:46-75 (sky resolve on stencil == 0)
public:
    SkyboxPass();
    const char* Name() const override { return "Skybox"; }
    void Execute(FGContext* context) override;
protected:
    ShadingState mShadingState;
};

class BloomPass : public ComputePass {   // :208-298
public:
    static constexpr uint32 BloomStep = 3;
    static constexpr uint32 MipmapLevel = BloomStep + 2;
    // halo_chain: {0, 0} = the mip chains have DeferredShadingRT's size (the reference); multi-GPU halo mode:
    // the size of the tile's extended rectangle E, on which the pyramid runs (the HDR target covers S = interior + 4 px)
    explicit BloomPass(RenderSize halo_chain = RenderSize{0, 0});
    const char* Name() const override { return "Bloom"; }
    void Execute(FGContext* context) override;
protected:
    ShadingState mDownsampleH[BloomStep], mDownsampleV[BloomStep], mUpsampleH[BloomStep], mUpsampleV[BloomStep];
    ShadingState mUpsampleBlurH, mUpsampleBlurV, mUpsampleMerge, mPrefilter;
    bool mHalo = false;
};

class ClusteredPass : public ComputePass {   // :300-369
public:
    static constexpr int32 ClusterSizeX = 24, ClusterSizeY = 16, ClusterSizeZ = 8;
    static constexpr int32 MaxSceneLights = 1024, MaxClusterLights = 32;
    ClusteredPass();
    const char* Name() const override { return "Clustered"; }
    void Execute(FGContext* context) override;
protected:
    ShadingState mClusteredCompute, mClusteredCulling;
    std::vector<pbr_light> mLights, mCommitted;   // this frame's light buffer / what the device buffer holds
    int mCommittedCount = -1;
};

class AutoExposurePass : public ComputePass {   // :371-429
public:
    static constexpr float MinLogLuminance = -10.0f, MaxLogLuminance = 2.0f;
    static constexpr float LogLuminanceRange = MaxLogLuminance - MinLogLuminance;
    static constexpr float InvLogLuminanceRange = 1.0f / (MaxLogLuminance - MinLogLuminance);
    static constexpr uint32 HistogramComputeThreadGroupSize = 16, HistogramBinSize = 256;
    AutoExposurePass();
    const char* Name() const override { return "AutoExposure"; }
    void Execute(FGContext* context) override;
    void SetInitialLuminance(float v) { mInitialLuminance = v; mAvarageLuminanceInitialized = false; }
    // multi-GPU: PixelCount of the WHOLE frame; 0 = this device's texture
    void SetFullFramePixelCount(uint32 n) { mFullFramePixels = n; }
protected:
    ShadingState mLuminanceHistogramCompute, mAvarageLuminanceCompute;
    bool mAvarageLuminanceInitialized;
    float mInitialLuminance = 0.0f;   // DeferredPipeline.cpp:268-274 initialises to 0 (quirk Q20)
    uint32 mFullFramePixels = 0;
};

class ToneMappingPass : public GraphicsPass {   // :431-461
public:
    explicit ToneMappingPass(RenderSize s);
    const char* Name() const override { return "ToneMapping"; }
    void Execute(FGContext* context) override;
protected:
    ShadingState mToneMappingRender;
};

// Not in the reference, which has no anti-aliasing: the integer edge filter pbr_fxaa on the tone-mapped target, into a texture of its
// own that becomes the presented one.  Part of the pipeline only while DeferredRenderPipeline::SetAntiAliasing is on.
class AntiAliasPass : public GraphicsPass {
public:
    static constexpr const char* Shader = "fxaa.hip";   // the binding-table row's name: no shader file of the reference
    AntiAliasPass();
    const char* Name() const override { return "AntiAlias"; }
    void Execute(FGContext* context) override;
    static FGTransientTextureDescription Target(RenderSize s) {
        return FGTransientTextureDescription{(uint16)s.Width, (uint16)s.Height, 1, ETextureFormat_R8G8B8A8_UNORM, ETexture2DFlag_AllowRenderTarget};
    }
protected:
    ShadingState mAntiAliasRender;
};

// Not in the reference, which computes a directional light (deferred_shading.hlsl:144-156) and never adds it, and has no shadows: the sun
// of pbr_sun_light.  SunShadowPass rasterizes the scene's meshes (GBufferPass's device copies: it runs after that pass) under the
// orthographic light camera pbr_sun_fit fits around the draws' world boxes, into the frame-graph texture SunShadowDepth — once per
// mesh upload / sun change, not per frame; SunLightPass adds the light to DeferredShadingRT after DeferredShading and the sky resolve
// and before Bloom.  Both are part of the pipeline only while DeferredRenderPipeline::SetSunLight has a sun.
struct SunSettings {
    float Direction[3] = {0, 1, 0};   // normalised by SetSunLight (double, rounded once)
    float Luminance[3] = {0, 0, 0};
    uint32 MapSize = 2048, Pcf = 3;
    float BiasConst = 0, BiasSlope = 0;
    bool Shadows = true;
    bool DepthOnly = false;           // the map by pbr_depth_raster (the same bits, no scratch planes) instead of pbr_gbuffer_raster
    uint64_t Serial = 0;              // bumped by every SetSunLight: the map is rasterized again
    float LightViewProj[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};   // written by SunShadowPass
};

class SunShadowPass : public GraphicsPass {
public:
    SunShadowPass(const GBufferPass* gbuffer, SunSettings* sun);
    const char* Name() const override { return "SunShadow"; }
    void Execute(FGContext* context) override;
    static FGTransientTextureDescription Target(uint32 map_size) {
        return FGTransientTextureDescription{(uint16)map_size, (uint16)map_size, 1, ETextureFormat_DepthStencil, ETexture2DFlag_AllowDepthStencil};
    }
    // the union of the draws' world boxes (the exact local min / max of each draw's valid triangles through its Model, in double,
    // rounded outwards): scene.world_box of the Python side, operation for operation.  false: no valid triangle
    static bool WorldBox(const MeshSource& meshes, pbr_aabb* out);
protected:
    const GBufferPass* mGBuffer;
    SunSettings* mSun;
    ShadingState mShadingState;
    // the raster's scratch and the A / B / C planes it writes and nobody reads (17 B per texel with the target's depth and stencil);
    // with SunSettings::DepthOnly there are no planes, and the scratch is the depth raster's
    std::unique_ptr<DeviceStructuredBuffer> mPlanes, mRasterScratch;
    uint64_t mUploadsSeen = ~0ull, mSerialSeen = ~0ull;
};

class SunLightPass : public GraphicsPass {
public:
    static constexpr const char* Shader = "sun_light.hip";   // the binding-table row's name: no shader file of the reference
    SunLightPass(SunSettings* sun, bool shadows);
    const char* Name() const override { return "SunLight"; }
    void Execute(FGContext* context) override;
protected:
    SunSettings* mSun;
    bool mShadows;
    ShadingState mShadingState;
};

class DeferredRenderPipeline : public IRenderPipeline {   // :463-481, DeferredPipeline.cpp:17-44
public:
    DeferredRenderPipeline(RenderSize size, uint32 env_size = PreFilterEnvMapPass::PreFilterEnvMapSize, uint32 lut_res = PrecomputeBRDFPass::TextureResolution)
        : mSize(size), mEnvSize(env_size), mLutRes(lut_res) {}
    // one device's tile of a larger frame: every target covers the layout's shaded rectangle S; in halo mode the
    // bloom chains cover the extended rectangle E
    DeferredRenderPipeline(const TileLayout& layout, uint32 env_size = PreFilterEnvMapPass::PreFilterEnvMapSize, uint32 lut_res = PrecomputeBRDFPass::TextureResolution)
        : mSize(RenderSize{layout.Shaded.w, layout.Shaded.h}), mEnvSize(env_size), mLutRes(lut_res),
          mHaloChain(layout.Halo ? RenderSize{layout.Bloom.w, layout.Bloom.h} : RenderSize{0, 0}) {}
    std::vector<IRenderPass*> Setup() override;
    // The pass list with (on) or without AntiAliasPass between ToneMapping and Present, and the present pass re-pointed at the
    // texture it shows; for FrameGraph::Recompile, after Setup.  Off (the default): exactly Setup()'s list.
    std::vector<IRenderPass*> SetAntiAliasing(bool on);
    bool AntiAliasing() const { return mAntiAliasing; }
    // The pass list with (on) or without SunShadowPass (shadows) and SunLightPass, for FrameGraph::Recompile; Bloom gets its order edge
    // behind SunLight, or loses it.  Off (the default): exactly Setup()'s list (with AntiAliasPass if that is on).
    // A failed call changes nothing.  A successful one keeps the passes it replaces alive — the frame graph still points at them —
    // until the caller has recompiled the graph with the returned list and calls CommitSunLight; if the recompile fails,
    // RollbackSunLight puts the earlier sun (or none) back and returns its list to recompile with.
    std::vector<IRenderPass*> SetSunLight(bool on, const SunSettings& sun = SunSettings{});
    void CommitSunLight();
    std::vector<IRenderPass*> RollbackSunLight();
    bool SunLight() const { return mSunLightPass != nullptr; }
    const SunSettings& Sun() const { return mSun; }
    RenderSize Size() const { return mSize; }

    std::unique_ptr<GBufferPass> mGBufferPass;
    std::unique_ptr<DeferredShadingPass> mDeferredShadingPass;
    std::unique_ptr<SkyboxPass> mSkyboxPass;
    std::unique_ptr<BloomPass> mBloomPass;
    std::unique_ptr<PreFilterEnvMapPass> mPrefilterEnvMapPass;
    std::unique_ptr<PrecomputeBRDFPass> mPrecomputeBRDFPass;
    std::unique_ptr<AutoExposurePass> mAutoExposurePass;
    std::unique_ptr<ToneMappingPass> mToneMappingPass;
    std::unique_ptr<ClusteredPass> mClusteredPass;
    std::unique_ptr<AntiAliasPass> mAntiAliasPass;   // null until anti-aliasing is first turned on
    std::unique_ptr<SunShadowPass> mSunShadowPass;   // null without a shadowed sun
    std::unique_ptr<SunLightPass> mSunLightPass;     // null without a sun
private:
    std::vector<IRenderPass*> mPasses;   // Setup()'s list
    std::vector<IRenderPass*> Compose() const;   // Setup()'s list + the optional passes that are on, Present last
    SunSettings mSun, mOldSun;
    std::unique_ptr<SunShadowPass> mOldSunShadowPass;   // between SetSunLight and CommitSunLight / RollbackSunLight
    std::unique_ptr<SunLightPass> mOldSunLightPass;
    bool mSunPending = false;
    bool mAntiAliasing = false;
    RenderSize mSize;
    uint32 mEnvSize, mLutRes;
    RenderSize mHaloChain{0, 0};
};

}  // namespace MRendererHip
