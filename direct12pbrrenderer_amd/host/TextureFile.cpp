// TextureFile.cpp — see TextureFile.h
#include "TextureFile.h"

#include <cstring>
#include <string>

#include "FrameGraphResource.h"

namespace MRendererHip {

pbr_texture2d ParseTextureFile(const uint8_t* file, size_t bytes) {
    constexpr size_t HEADER = 16;   // TextureInfo (12) + the payload's byte count (4)
    if (!file || bytes < HEADER) throw HipException("texture file: truncated header");
    uint16_t info[4];               // width, height, depth, mips (little-endian, as the reference's writer leaves them)
    std::memcpy(info, file, sizeof(info));
    const uint8_t format = file[8];
    uint32_t payload;
    std::memcpy(&payload, file + 12, sizeof(payload));
    if (info[2] != 1) throw HipException("texture file: depth " + std::to_string(info[2]) + " (2D textures only)");
    if (format != PBR_TEX_R8G8B8A8_UNORM && format != PBR_TEX_B8G8R8A8_UNORM && format != PBR_TEX_B8G8R8A8_UNORM_SRGB &&
        format != PBR_TEX_R8_UNORM)
        throw HipException("texture file: unknown format " + std::to_string(format));
    pbr_texture2d t{file + HEADER, info[0], info[1], info[3], (uint32_t)format | PBR_TEX_BC1_BLOCKS};
    const size_t want = pbr_texture2d_bytes(t.width, t.height, t.mip_levels, t.format);
    if (!want) throw HipException("texture file: bad size or level count");
    if (payload != want)
        throw HipException("texture file: payload of " + std::to_string(payload) + " bytes, the BC1 chain takes " + std::to_string(want));
    if (bytes - HEADER < payload) throw HipException("texture file: truncated payload");
    if (bytes - HEADER > payload) throw HipException("texture file: bytes after the payload");
    return t;
}

size_t WriteTextureFile(const pbr_texture2d& t, uint8_t* file, size_t bytes) {
    constexpr size_t HEADER = 16;
    if (!(t.format & PBR_TEX_BC1_BLOCKS)) throw HipException("texture file: the chain to write is not BC1 blocks (PBR_TEX_BC1_BLOCKS)");
    const size_t payload = pbr_texture2d_bytes(t.width, t.height, t.mip_levels, t.format);
    if (!payload) throw HipException("texture file: bad size, level count or format");
    if (!file) return HEADER + payload;
    if (!t.texels) throw HipException("texture file: null blocks");
    if (bytes < HEADER + payload) throw HipException("texture file: output buffer too small");
    const uint16_t info[4] = {(uint16_t)t.width, (uint16_t)t.height, 1, (uint16_t)t.mip_levels};   // (sizes are <= PBR_TEX_MAX_SIZE)
    const uint32_t count = (uint32_t)payload;
    std::memcpy(file, info, sizeof(info));
    file[8] = (uint8_t)(t.format & 0xffu);
    file[9] = file[10] = file[11] = 0;
    std::memcpy(file + 12, &count, sizeof(count));
    std::memcpy(file + HEADER, t.texels, payload);
    return HEADER + payload;
}

}  // namespace MRendererHip
