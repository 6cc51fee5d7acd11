// HdrImage.h — Radiance .hdr (RGBE) file ingestion for sky cubes.
//
// Reference: ResourceLoader::LoadHDRImageFile / LoadCubeMap (Engine/Source/Resource/ResourceLoader.cpp:381-428)
// hand the six faces px/nx/py/ny/pz/nz.hdr to DirectX::LoadFromHDRFile and then to GenerateMipMaps
// (:465-507).  DirectXTex is an un-vendored vcpkg dependency; the parser below follows the published file
// format (Radiance "picture" files: text header, "-Y h +X w" resolution line, flat or new-style
// run-length-encoded RGBE scanlines).  Split of work: the byte-serial parse and RLE expansion stay on the
// host (a face is <= a few MB), the RGBE -> fp32 conversion and the mip chain run on the GPU
// (pbr_rgbe_decode, pbr_cube_gen_mips).
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "Scene.h"

namespace MRendererHip {

struct HdrImage {
    uint32_t Width = 0, Height = 0;
    std::vector<uint8_t> Rgbe;   // Width * Height * 4, rows top to bottom
};

// Parses a whole .hdr file held in memory.  Throws HipException with a reason on malformed input
// (bad magic, unsupported FORMAT / orientation, truncated or inconsistent scanline data).
HdrImage ParseRadianceHDR(const uint8_t* file, size_t bytes);
HdrImage LoadHDRImageFile(const std::string& path);

// The file half of LoadCubeMap: the six faces parsed and checked (square, equal, a multiple of 4 texels); returns their size.
uint32_t LoadCubeMapFaces(const std::string& dir, HdrImage (&faces)[6]);

// LoadCubeMap (ResourceLoader.cpp:408-428): <dir>/{px,nx,py,ny,pz,nz}.hdr -> fp32 RGBA cube with the full box
// mip chain and its SH9 pack.  Faces must be square, equal, and a multiple of 4 texels (:399-403).
std::shared_ptr<SkyBox> LoadCubeMap(pbr_ctx* ctx, const std::string& dir);

// An equirectangular (latitude-longitude) panorama in host memory as the source of a cube's level 0: Width x Height texels, rows top
// to bottom, fp32 RGBA (16 bytes a texel) or, with Rgbe, Radiance texels (4 bytes) that the kernel decodes where it fetches them.
// The reference takes faces only; the resampling rule is pbr_equirect_to_cube's (include/pbr_hip.h).
struct Panorama {
    const void* Texels = nullptr;
    uint32_t Width = 0, Height = 0;
    bool Rgbe = false;
};
// size 0 / samples 0 -> what the default rules pick for the panorama (pbr_equirect_default_size / _samples)
void EquirectDefaults(const Panorama& pano, uint32_t& size, uint32_t& samples);
// Uploads the panorama as it is and resamples it into cube_level0 (device, 6 size^2 float4) on ctx.  Blocks until the GPU is done
// (the uploaded copy is released on return).  Throws HipException with pbr_equirect_to_cube's reason for what it refuses.
void PanoramaToCube(pbr_ctx* ctx, const Panorama& pano, float* cube_level0, uint32_t size, uint32_t samples);
// LoadCubeMap for one equirectangular .hdr of any aspect ratio: its RGBE texels are uploaded and sampled in place into a cube of
// `size` (0: the default rule) with `samples`^2 sub-samples a texel (0: the default rule), then the full box mip chain and the SH9 pack.
std::shared_ptr<SkyBox> LoadEquirectSkyBox(pbr_ctx* ctx, const std::string& hdr_path, uint32_t size, uint32_t samples);

}  // namespace MRendererHip
