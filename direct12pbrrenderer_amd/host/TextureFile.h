// TextureFile.h — the reference's serialized 2D texture (a texture asset's _data.bin), read as it is: from the file to a BC1-resident
// pbr_texture2d with no CPU decode; and written from one (the file half of TextureData::BinarySerialize, BasicStorage.cpp:161-171).
//
// Reference: a texture resource is a binary blob (Engine/Include/Resource/BasicStorage.h:193-233): TextureInfo
//     uint16 mWidth, mHeight, mDepth, mMipmap;  uint8 mFormat (the DXGI number);  3 pad bytes          (12 bytes)
// then a uint32 payload byte count at offset 12 and the payload at offset 16.  The payload of the scene's textures is the whole
// mip chain as BC1 blocks (level i: max(1, ((w >> i) + 3) / 4) x max(1, ((h >> i) + 3) / 4) blocks of 8 bytes, levels
// concatenated), and mFormat is the format the reference decodes them into at load time (TextureDecompressInternal,
// TextureCompression.cpp).  That payload is the layout of a pbr_texture2d with PBR_TEX_BC1_BLOCKS (include/pbr_hip.h) byte
// for byte: it can be uploaded and sampled in place, or decoded on the GPU by pbr_bc1_decode.
#pragma once
#include <cstddef>
#include <cstdint>

#include "pbr_hip.h"

namespace MRendererHip {

// Parses a whole texture file held in memory.  Returns its description: format = the stored format | PBR_TEX_BC1_BLOCKS,
// texels = the payload inside `file` (bytes: pbr_texture2d_bytes of the description).  Stateless.
// Throws HipException with a reason: a truncated file, a byte count that disagrees with the file's size or with
// pbr_texture2d_bytes, depth != 1, an unknown format, a size or level count the library refuses.
pbr_texture2d ParseTextureFile(const uint8_t* file, size_t bytes);

// The inverse: the file of a BC1 chain.  t: format = the stored format | PBR_TEX_BC1_BLOCKS, texels = the chain's blocks (host,
// pbr_texture2d_bytes of the description).  Writes TextureInfo, the byte count and the payload to `file` and returns the file's
// size, 16 + pbr_texture2d_bytes; with file == nullptr only the size (texels is not read).  Stateless.
// Throws HipException with a reason: a description without PBR_TEX_BC1_BLOCKS or one pbr_texture2d_bytes rejects, null blocks, a
// buffer smaller than the file.
size_t WriteTextureFile(const pbr_texture2d& t, uint8_t* file, size_t bytes);

}  // namespace MRendererHip
