// CubeMapFile.h — the reference's serialized sky cube (a CubeMapResource's data file), read as it is: from the file to the device with
// no CPU decode — the six BC6H_UF16 chains are decoded in place on the GPU (pbr_bc6h_decode_cube); and written from six chains.
//
// Reference: CubeMapTextureData is reflected as mData, then mSHCoefficients (Utils/ReflectionDef.h:81-84), and a reflected class
// writes its serializable fields one after the other and nothing else — no tag, no count, no padding (Utils/Serialization.h:175-204;
// read back the same way, :206-236).  mData is a std::array of six TextureData, serialized element after element without a count
// (Serialization.h:128-147); each TextureData through its own BinarySerialize (BasicStorage.cpp:161-171; read: :173-188):
//     TextureInfo  uint16 mWidth, mHeight, mDepth, mMipmap;  uint8 mFormat (the DXGI number);  3 pad bytes             (12 bytes)
//     uint32       the payload's byte count
//     payload      the face's whole mip chain as BC6H blocks (every HDR texture is stored as DXGI_FORMAT_BC6H_UF16:
//                  TextureCompression.h:13-14): level i is max(1, ((w >> i) + 3) / 4)^2 blocks of 16 bytes, levels concatenated
// mFormat is the format the reference decodes into, one of its HDR formats (TextureCompressor::IsHDRFormat, TextureCompression.cpp:
// 6-10: DXGI 1 .. 18).  Then SH2CoefficientsPack (ReflectionDef.h:45-53, Utils/SH.h:20-29): seven Vector4, each reflected as its
// four floats x, y, z, w (ReflectionDef.h:29-34, arithmetic fields as their bytes: Serialization.h:57-62) — 112 bytes in
// pbr_sh_pack's order.  A payload is a multiple of 16 bytes, so every face's payload starts at a multiple of 16 from the file's
// start: face f at 16 + f (16 + payload).  Faces in the reference's order px, nx, py, ny, pz, nz (ResourceLoader.cpp:415).
#pragma once
#include <cstddef>
#include <cstdint>

#include <memory>
#include <string>

#include "pbr_hip.h"

namespace MRendererHip {

struct SkyBox;

struct CubeMapFileInfo {
    uint32_t Size = 0, MipLevels = 0;
    uint8_t Format = 0;             // the DXGI number the reference decodes into (1 .. 18)
    size_t FaceOffset[6] = {};      // byte offset of each face's payload in the file; each holds pbr_bc6h_chain_bytes(Size, MipLevels)
    pbr_sh_pack SH{};
};

// Parses a whole cube-map file held in memory.  Stateless.  Throws HipException with a reason: a truncated file, faces whose
// TextureInfo differ, width != height, depth != 1, a format outside the reference's HDR range, a byte count that disagrees with
// pbr_bc6h_chain_bytes or with the file's size.
CubeMapFileInfo ParseCubeMapFile(const uint8_t* file, size_t bytes);

// The inverse: six host chains of blocks (pbr_bc6h_chain_bytes(size, mip_levels) bytes each) and a pack -> the file.  format: the
// DXGI number written into every TextureInfo (the reference's sky imports are R32G32B32A32_FLOAT: 2).  Returns the file's size,
// 6 (16 + chain bytes) + 112; with file == nullptr only the size (faces is not read).  Throws HipException with a reason: a size or
// level count pbr_bc6h_chain_bytes rejects, a format outside the HDR range, a null face, a buffer smaller than the file.
size_t WriteCubeMapFile(const void* const faces[6], uint32_t size, uint32_t mip_levels, uint8_t format, const pbr_sh_pack& sh,
                        uint8_t* file, size_t bytes);

// CubeMapResource's load (ResourceDef.cpp:187-219) on the GPU: the file is uploaded as it is, its six chains are decoded in place on
// ctx into an fp32 RGBA cube with the file's own levels (pbr_bc6h_decode_cube), and the SH pack is the file's, as the reference takes
// it (ResourceDef.cpp:211), or with recompute_sh pbr_sh9_project of the decoded level 0.  Blocks until the GPU is done.
std::shared_ptr<SkyBox> SkyBoxFromCubeMapFile(pbr_ctx* ctx, const uint8_t* file, size_t bytes, bool recompute_sh, bool resident = false);
// the same for a file on disk
std::shared_ptr<SkyBox> LoadCubeMapFile(pbr_ctx* ctx, const std::string& path, bool recompute_sh, bool resident = false);


// ResourceLoader::ImportCubeMap (ResourceLoader.cpp:279-299) on the GPU, from decoded faces on: level 0 — cube_mip0 (host, 6 x size^2
// fp32 RGBA) or, when rgbe_faces is given, six parsed .hdr faces expanded by pbr_rgbe_decode — is uploaded, its box mips made
// (pbr_cube_gen_mips), the SH pack projected from the fp32 level 0 BEFORE compression (where the reference computes it, in the
// CubeMapTextureData constructor, BasicStorage.h:313), the chain compressed (pbr_bc6h_encode_cube_ex with `flags`: 0, or
// PBR_BC6H_ENCODE_TWO_REGION for the two-region modes as well), read back and written by WriteCubeMapFile with format 2.
// mip_levels 0 = the full chain.  Returns the file's size; with file == nullptr only the size, and nothing runs.  Blocks until the GPU is done.  Throws HipException: a size or level count pbr_bc6h_chain_bytes rejects, a null
// level 0, a buffer smaller than the file, an unknown flag.
// pano: a third kind of level-0 source (not the reference's, which takes faces only) — an equirectangular panorama, uploaded as it is
// and resampled into level 0 by pbr_equirect_to_cube with `samples`^2 sub-samples a texel; size 0 / samples 0: the default rules
// (EquirectDefaults).  The size query reads pano's Width only (Texels may be null).  Everything after level 0 is the same.
struct HdrImage;
struct Panorama;
size_t ImportCubeMap(pbr_ctx* ctx, const float* cube_mip0, const HdrImage* rgbe_faces, uint32_t size, uint32_t mip_levels,
                     uint8_t* file, size_t bytes, uint32_t flags = 0, const Panorama* pano = nullptr, uint32_t samples = 0);

}  // namespace MRendererHip
