// CubeMapFile.cpp — see CubeMapFile.h
#include "CubeMapFile.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "FrameGraphResource.h"
#include "HdrImage.h"
#include "Scene.h"

namespace MRendererHip {

namespace {
constexpr size_t HEADER = 16;       // TextureInfo (12) + the payload's byte count (4)
constexpr size_t SH_BYTES = sizeof(pbr_sh_pack);
static_assert(SH_BYTES == 112, "SH2CoefficientsPack is seven float4");
bool hdr_format(uint32_t f) { return f >= 1 && f <= 18; }   // R32G32B32A32_TYPELESS .. R32G32_SINT (TextureCompression.cpp:6-10)
}  // namespace

CubeMapFileInfo ParseCubeMapFile(const uint8_t* file, size_t bytes) {
    if (!file || bytes < HEADER) throw HipException("cube-map file: truncated header");
    CubeMapFileInfo out;
    size_t at = 0, chain = 0;
    uint16_t first[4] = {};
    for (int f = 0; f < 6; f++) {
        const std::string face = "cube-map file: face " + std::to_string(f) + ": ";
        if (bytes - at < HEADER) throw HipException(face + "truncated header");
        uint16_t info[4];           // width, height, depth, mips (little-endian, as the reference's writer leaves them)
        std::memcpy(info, file + at, sizeof(info));
        const uint8_t format = file[at + 8];
        uint32_t payload;
        std::memcpy(&payload, file + at + 12, sizeof(payload));
        if (f == 0) {
            if (info[0] != info[1]) throw HipException(face + std::to_string(info[0]) + " x " + std::to_string(info[1]) + " (cube faces are square)");
            if (info[2] != 1) throw HipException(face + "depth " + std::to_string(info[2]) + " (2D faces only)");
            if (!hdr_format(format)) throw HipException(face + "format " + std::to_string(format) + " is not one of the reference's HDR formats (1 .. 18)");
            chain = pbr_bc6h_chain_bytes(info[0], info[3]);
            if (!chain) throw HipException(face + "bad size or level count (" + std::to_string(info[0]) + ", " + std::to_string(info[3]) + " levels)");
            std::memcpy(first, info, sizeof(first));
            out.Size = info[0]; out.MipLevels = info[3]; out.Format = format;
        } else if (std::memcmp(first, info, sizeof(first)) != 0 || format != out.Format) {
            throw HipException(face + "its TextureInfo differs from face 0's");
        }
        if (payload != chain)
            throw HipException(face + "payload of " + std::to_string(payload) + " bytes, the BC6H chain takes " + std::to_string(chain));
        if (bytes - at - HEADER < payload) throw HipException(face + "truncated payload");
        out.FaceOffset[f] = at + HEADER;
        at += HEADER + payload;
    }
    if (bytes - at < SH_BYTES) throw HipException("cube-map file: truncated SH coefficients");
    if (bytes - at > SH_BYTES) throw HipException("cube-map file: bytes after the SH coefficients");
    std::memcpy(&out.SH, file + at, SH_BYTES);
    return out;
}

size_t WriteCubeMapFile(const void* const faces[6], uint32_t size, uint32_t mip_levels, uint8_t format, const pbr_sh_pack& sh,
                        uint8_t* file, size_t bytes) {
    const size_t chain = pbr_bc6h_chain_bytes(size, mip_levels);
    if (!chain) throw HipException("cube-map file: bad size or level count");
    if (!hdr_format(format)) throw HipException("cube-map file: format " + std::to_string(format) + " is not one of the reference's HDR formats (1 .. 18)");
    const size_t total = 6 * (HEADER + chain) + SH_BYTES;
    if (!file) return total;
    if (!faces) throw HipException("cube-map file: null faces");
    for (int f = 0; f < 6; f++)
        if (!faces[f]) throw HipException("cube-map file: null face " + std::to_string(f));
    if (bytes < total) throw HipException("cube-map file: output buffer too small");
    const uint16_t info[4] = {(uint16_t)size, (uint16_t)size, 1, (uint16_t)mip_levels};   // (size <= PBR_BC6H_MAX_SIZE)
    const uint32_t count = (uint32_t)chain;
    size_t at = 0;
    for (int f = 0; f < 6; f++) {
        std::memcpy(file + at, info, sizeof(info));
        file[at + 8] = format;
        file[at + 9] = file[at + 10] = file[at + 11] = 0;
        std::memcpy(file + at + 12, &count, sizeof(count));
        std::memcpy(file + at + HEADER, faces[f], chain);
        at += HEADER + chain;
    }
    std::memcpy(file + at, &sh, SH_BYTES);
    return total;
}

// resident: the uploaded file IS the sky (SkyBox::Blocks); no decoded cube outlives this call
static std::shared_ptr<SkyBox> ResidentSkyBox(pbr_ctx* ctx, const uint8_t* file, size_t bytes, const CubeMapFileInfo& info, bool recompute_sh) {
    auto check = [&](pbr_status st) { if (st != PBR_OK) throw HipException(pbr_last_error(ctx)); };
    auto sky = std::make_shared<SkyBox>();
    sky->Blocks = std::make_shared<DeviceBc6hCube>(info.Size, info.MipLevels, file, bytes, info.FaceOffset);
    sky->SH = info.SH;
    if (recompute_sh) {             // the projection of the decoded level 0: one level into a transient cube
        DeviceTexture2DArray level0(info.Size, 1, ETextureFormat_R32G32B32A32_FLOAT);
        DeviceStructuredBuffer pack(112, 4);
        const pbr_cube_bc6h b = sky->Blocks->Blocks();
        check(pbr_bc6h_decode_cube(ctx, b.face_blocks, info.Size, 1, (float*)level0.DevicePtr()));
        pbr_cube_f32 c{(const float*)level0.DevicePtr(), info.Size, 1};
        check(pbr_sh9_project(ctx, &c, (float*)pack.DevicePtr()));
        check(pbr_sync(ctx));       // `level0` is released on return
        ThrowIfFailed(hipMemcpy(&sky->SH, pack.DevicePtr(), 112, hipMemcpyDeviceToHost), "read SH");
    }
    return sky;
}

std::shared_ptr<SkyBox> SkyBoxFromCubeMapFile(pbr_ctx* ctx, const uint8_t* file, size_t bytes, bool recompute_sh, bool resident) {
    const CubeMapFileInfo info = ParseCubeMapFile(file, bytes);
    if (resident) return ResidentSkyBox(ctx, file, bytes, info, recompute_sh);
    auto check = [&](pbr_status st) { if (st != PBR_OK) throw HipException(pbr_last_error(ctx)); };
    DeviceMemory staged(bytes);     // (hipMalloc is 256-byte aligned, so every payload is 16-byte aligned on the device too)
    // (a blocking copy from pageable memory has landed when it returns: the context's stream needs no event to see it)
    ThrowIfFailed(hipMemcpy(staged.Ptr(), file, bytes, hipMemcpyHostToDevice), "upload cube-map file");
    const void* faces[6];
    for (int f = 0; f < 6; f++) faces[f] = (const uint8_t*)staged.Ptr() + info.FaceOffset[f];
    auto sky = std::make_shared<SkyBox>();
    sky->Cube = std::make_shared<DeviceTexture2DArray>(info.Size, info.MipLevels, ETextureFormat_R32G32B32A32_FLOAT);
    check(pbr_bc6h_decode_cube(ctx, faces, info.Size, info.MipLevels, (float*)sky->Cube->DevicePtr()));
    if (recompute_sh) {
        DeviceStructuredBuffer pack(112, 4);
        pbr_cube_f32 c{(const float*)sky->Cube->DevicePtr(), info.Size, info.MipLevels};
        check(pbr_sh9_project(ctx, &c, (float*)pack.DevicePtr()));
        check(pbr_sync(ctx));
        ThrowIfFailed(hipMemcpy(&sky->SH, pack.DevicePtr(), 112, hipMemcpyDeviceToHost), "read SH");
    } else {
        check(pbr_sync(ctx));       // `staged` is released on return
        sky->SH = info.SH;
    }
    return sky;
}

std::shared_ptr<SkyBox> LoadCubeMapFile(pbr_ctx* ctx, const std::string& path, bool recompute_sh, bool resident) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) throw HipException("cube-map file: cannot open " + path);
    std::vector<uint8_t> data;
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + n);
    std::fclose(f);
    try {
        return SkyBoxFromCubeMapFile(ctx, data.data(), data.size(), recompute_sh, resident);
    } catch (const HipException& e) {
        throw HipException(path + ": " + e.what());
    }
}

size_t ImportCubeMap(pbr_ctx* ctx, const float* cube_mip0, const HdrImage* rgbe_faces, uint32_t size, uint32_t mip_levels,
                     uint8_t* file, size_t bytes, uint32_t flags, const Panorama* pano, uint32_t samples) {
    if (flags & ~PBR_BC6H_ENCODE_TWO_REGION) throw HipException("cube-map import: unknown flag");
    if (pano) {
        if (!pano->Width || !pano->Height || pano->Width > PBR_EQUIRECT_MAX_W || pano->Height > PBR_EQUIRECT_MAX_H)
            throw HipException("cube-map import: a panorama of " + std::to_string(pano->Width) + " x " + std::to_string(pano->Height) + " texels");
        EquirectDefaults(*pano, size, samples);
        if (samples != 1 && samples != 2 && samples != 4 && samples != 8) throw HipException("cube-map import: samples not 0, 1, 2, 4 or 8");
    }
    if (mip_levels == 0)
        for (uint32_t s = size; s; s >>= 1) mip_levels++;
    const size_t chain = pbr_bc6h_chain_bytes(size, mip_levels);
    if (!chain) throw HipException("cube-map import: bad size or level count (" + std::to_string(size) + ", " + std::to_string(mip_levels) + " levels)");
    const size_t total = WriteCubeMapFile(nullptr, size, mip_levels, 2, pbr_sh_pack{}, nullptr, 0);
    if (!file) return total;
    if (!cube_mip0 && !rgbe_faces && !(pano && pano->Texels)) throw HipException("cube-map import: null level 0");
    if (bytes < total) throw HipException("cube-map import: output buffer too small");
    auto check = [&](pbr_status st) { if (st != PBR_OK) throw HipException(pbr_last_error(ctx)); };
    const size_t face_texels = (size_t)size * size;
    DeviceMemory cube(pbr_cube_texels(size, mip_levels) * 16), blocks(6 * chain), pack(SH_BYTES);
    // (a blocking copy from pageable memory has landed when it returns: the context's stream needs no event to see it)
    if (pano) {
        PanoramaToCube(ctx, *pano, (float*)cube.Ptr(), size, samples);
    } else if (rgbe_faces) {
        DeviceMemory staging(6 * face_texels * 4);
        for (int f = 0; f < 6; f++)
            ThrowIfFailed(hipMemcpy((uint8_t*)staging.Ptr() + f * face_texels * 4, rgbe_faces[f].Rgbe.data(), face_texels * 4, hipMemcpyHostToDevice), "upload rgbe face");
        check(pbr_rgbe_decode(ctx, (const uint8_t*)staging.Ptr(), 6 * face_texels, (float*)cube.Ptr()));
        check(pbr_sync(ctx));       // `staging` is released here
    } else {
        ThrowIfFailed(hipMemcpy(cube.Ptr(), cube_mip0, 6 * face_texels * 16, hipMemcpyHostToDevice), "upload level 0");
    }
    if (mip_levels > 1) check(pbr_cube_gen_mips(ctx, (float*)cube.Ptr(), size, mip_levels));
    pbr_cube_f32 c{(const float*)cube.Ptr(), size, mip_levels};
    check(pbr_sh9_project(ctx, &c, (float*)pack.Ptr()));
    void* faces_dev[6];             // (hipMalloc is 256-byte aligned and a chain is a multiple of 16 bytes)
    for (int f = 0; f < 6; f++) faces_dev[f] = (uint8_t*)blocks.Ptr() + f * chain;
    check(pbr_bc6h_encode_cube_ex(ctx, (const float*)cube.Ptr(), size, mip_levels, faces_dev, flags));
    check(pbr_sync(ctx));
    std::vector<uint8_t> host(6 * chain);
    pbr_sh_pack sh{};
    ThrowIfFailed(hipMemcpy(host.data(), blocks.Ptr(), host.size(), hipMemcpyDeviceToHost), "read blocks");
    ThrowIfFailed(hipMemcpy(&sh, pack.Ptr(), SH_BYTES, hipMemcpyDeviceToHost), "read SH");
    const void* faces_host[6];
    for (int f = 0; f < 6; f++) faces_host[f] = host.data() + f * chain;
    return WriteCubeMapFile(faces_host, size, mip_levels, 2, sh, file, bytes);
}

}  // namespace MRendererHip
