"""ctypes / numpy mirrors of the POD structs in include/pbr_hip.h.

Each struct cites the reference type it mirrors (paths relative to /root/reference).
"""
import ctypes as C

import numpy as np

CLUSTER_X, CLUSTER_Y, CLUSTER_Z = 24, 16, 8          # DeferredRendering/Shader/clustered.hlsli:10-12
MAX_LIGHTS_PER_CLUSTER = 32                           # clustered.hlsli:9
MAX_SCENE_LIGHTS = 1024                               # Engine/Include/Renderer/Pipeline/DeferredPipeline.h:329
NUM_CLUSTERS = CLUSTER_X * CLUSTER_Y * CLUSTER_Z
HISTOGRAM_BINS = 256                                  # DeferredPipeline.h:409
ENV_MIPS = 5                                          # global.hlsli:9
BLOOM_MIPS = 5                                        # DeferredPipeline.h:212
# AutoExposurePass constants, DeferredPipeline.h:404-407
MIN_LOG_LUMINANCE = -10.0
MAX_LOG_LUMINANCE = 2.0
LOG_LUMINANCE_RANGE = MAX_LOG_LUMINANCE - MIN_LOG_LUMINANCE
INV_LOG_LUMINANCE_RANGE = float(np.float32(1.0) / np.float32(LOG_LUMINANCE_RANGE))
# BloomPass prefilter constants, DeferredPipeline.cpp:419-420
BLOOM_THRESHOLD = 1.0
BLOOM_KNEE = 0.5


class ShPack(C.Structure):
    """SH2CoefficientsPack, Engine/Include/Utils/SH.h:20-29."""
    _fields_ = [(n, C.c_float * 4) for n in ("sha_r", "shb_r", "sha_g", "shb_g", "sha_b", "shb_b", "shc")]


class Global(C.Structure):
    """ConstantBufferGlobal, Engine/Include/Renderer/Pipeline/IPipeline.h:38-62."""
    _fields_ = [
        ("SkyBoxSH", ShPack),
        ("InvView", C.c_float * 16),
        ("View", C.c_float * 16),
        ("Projection", C.c_float * 16),
        ("InvProjection", C.c_float * 16),
        ("CameraPos", C.c_float * 3),
        ("Ratio", C.c_float),
        ("Resolution", C.c_float * 2),
        ("Near", C.c_float),
        ("Far", C.c_float),
        ("Fov", C.c_float),
        ("DeltaTime", C.c_float),
        ("Time", C.c_float),
    ]


assert C.sizeof(Global) == 412


class Tile(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("x0", "y0", "w", "h", "full_w", "full_h")]


class ShadeTables(C.Structure):
    """pbr_shade_tables: the device buffer of the shade tables and the HOST descriptor of what its two halves were built for."""
    _fields_ = [("dev", C.c_void_p), ("bytes", C.c_uint64), ("built", C.c_uint32), ("num_lights", C.c_int32), ("list_pad", C.c_uint32), ("tile", Tile)]


# dword offsets into the shade tables' buffer (include/pbr_hip.h: PBR_TABLES_*)
TABLES_HEADER, TABLES_PLANES, TABLES_LISTS, TABLES_GEOM = 0, 4, 9232, 113680
TABLES_BUILT_FRAME, TABLES_BUILT_GEOMETRY = 1, 2


class GBuffer(C.Structure):
    """G-buffer planes (gbuffer.hlsl:10-26,144-146; formats DeferredPipeline.h:107-110)."""
    _fields_ = [
        ("A", C.c_void_p),
        ("B", C.c_void_p),
        ("C", C.c_void_p),
        ("depth", C.c_void_p),
        ("stencil", C.c_void_p),
        ("pitch", C.c_uint32),
    ]


class ShadeDesc(C.Structure):
    """pbr_shade_desc: one single-view shade launch (include/pbr_hip.h); pointers first, then the 32-bit fields: no padding.
    g, tile, gb and tables are HOST addresses (ctypes.addressof of a Global, Tile, GBuffer, ShadeTables the caller keeps alive)."""
    _fields_ = ([(n, C.c_void_p) for n in ("g", "tile", "gb", "lut", "lut_fold", "env_padded", "clusters", "lights", "hdr", "rects", "tables")]
                + [("lut_res", C.c_uint32), ("env_size", C.c_uint32), ("env_mips", C.c_uint32), ("num_lights", C.c_int32),
                   ("hdr_pitch", C.c_uint32), ("n_rects", C.c_uint32)])


class RasterDesc(C.Structure):
    """pbr_raster_desc: one G-buffer raster call (include/pbr_hip.h); 8-byte fields first, then the 32-bit ones: no padding.
    g, tile and textures are HOST addresses (of a Global, a Tile and a Texture2D array the caller keeps alive); maps, textures and
    n_textures unset: the constant-material raster; bounds and stats unset: no model cull."""
    _fields_ = ([(n, C.c_void_p) for n in ("g", "tile", "vertices", "indices", "draws", "A", "B", "C", "depth", "stencil", "scratch")]
                + [("scratch_bytes", C.c_size_t)] + [(n, C.c_void_p) for n in ("maps", "textures", "bounds", "stats")]
                + [(n, C.c_uint32) for n in ("n_vertices", "n_indices", "n_draws", "max_triangles", "pitch", "n_textures")])


class DepthRasterDesc(C.Structure):
    """pbr_depth_raster_desc: one depth-only raster call (include/pbr_hip.h); 8-byte fields first, then the 32-bit ones: no padding.
    g and tile are HOST addresses (of a Global and a Tile the caller keeps alive); bounds and stats unset: no model cull; reserved
    stays 0."""
    _fields_ = ([(n, C.c_void_p) for n in ("g", "tile", "vertices", "indices", "draws", "depth", "scratch")]
                + [("scratch_bytes", C.c_size_t)] + [(n, C.c_void_p) for n in ("bounds", "stats")]
                + [(n, C.c_uint32) for n in ("n_vertices", "n_indices", "n_draws", "max_triangles", "pitch", "reserved")])


class BloomDesc(C.Structure):
    """pbr_bloom_desc: one pbr_bloom call (include/pbr_hip.h); pointers first, then the 32-bit fields: no padding.  The three
    rectangles are HOST addresses of uint32[4] arrays the caller keeps alive; hdr_rect unset: the whole-image form; reserved stays 0."""
    _fields_ = ([(n, C.c_void_p) for n in ("hdr", "chain_a", "chain_b", "hist256", "hdr_rect", "merge_rect", "hist_rect")]
                + [(n, C.c_uint32) for n in ("w", "h", "hdr_pitch")]
                + [(n, C.c_float) for n in ("threshold", "knee", "min_log", "inv_range")] + [("reserved", C.c_uint32)])


class BloomPrefilterDesc(C.Structure):
    """pbr_bloom_prefilter_desc: one pbr_bloom_prefilter call (include/pbr_hip.h); pointers first, then the 32-bit fields: no padding.
    rects is the HOST address of a uint32[n_rects][4] array the caller keeps alive; unset with n_rects 0: the whole image into a
    dense plane; reserved stays 0."""
    _fields_ = ([(n, C.c_void_p) for n in ("hdr", "out", "rects")]
                + [(n, C.c_uint32) for n in ("w", "h", "pitch", "out_pitch", "out_x", "out_y", "n_rects")]
                + [(n, C.c_float) for n in ("threshold", "knee")] + [("reserved", C.c_uint32)])


MAX_VIEWS = 16                                        # PBR_MAX_VIEWS (include/pbr_hip.h)


class View(C.Structure):
    """pbr_view: the per-view camera and device buffers of a multi-view call (include/pbr_hip.h)."""
    _fields_ = [
        ("g", Global),
        ("gb", GBuffer),
        ("lights", C.c_void_p),
        ("num_lights", C.c_int32),
        ("clusters", C.c_void_p),
        ("hdr", C.c_void_p),
        ("hdr_pitch", C.c_uint32),
        ("chain_a", C.c_void_p),
        ("chain_b", C.c_void_p),
        ("hist256", C.c_void_p),
        ("avg", C.c_void_p),
        ("rgba8", C.c_void_p),
        ("out_pitch", C.c_uint32),
    ]


class FxaaImage(C.Structure):
    """pbr_fxaa_image: one image of a pbr_fxaa_batch call (device pointers, pitches in pixels)."""
    _fields_ = [("src", C.c_void_p), ("src_pitch", C.c_uint32), ("dst", C.c_void_p), ("dst_pitch", C.c_uint32)]


class Sun(C.Structure):
    """pbr_sun: the directional light of pbr_sun_light (HOST struct, 100 B): Direction is unit, from the surface towards the light."""
    _fields_ = [("Direction", C.c_float * 3), ("Luminance", C.c_float * 3), ("LightViewProj", C.c_float * 16),
                ("bias_const", C.c_float), ("bias_slope", C.c_float), ("pcf", C.c_uint32)]


class SunDesc(C.Structure):
    """pbr_sun_desc: one pbr_sun_light launch; pointers first, then the 32-bit fields: no padding.  g, tile, gb and sun are HOST
    addresses (ctypes.addressof of a Global, Tile, GBuffer, Sun the caller keeps alive); exactly one of hdr / contrib_f32."""
    _fields_ = ([(n, C.c_void_p) for n in ("g", "tile", "gb", "sun", "shadow_depth", "hdr", "contrib_f32")]
                + [(n, C.c_uint32) for n in ("map_w", "map_h", "map_pitch", "hdr_pitch")])


assert C.sizeof(Sun) == 100 and C.sizeof(SunDesc) == 72


class Aabb(C.Structure):
    """pbr_aabb as a HOST struct (pbr_sun_fit's world box); AABB_DTYPE is the same record for device arrays."""
    _fields_ = [("min", C.c_float * 3), ("max", C.c_float * 3)]


class HaloPeer(C.Structure):
    """pbr_halo_peer: rectangles {x, y, w, h} of the level-1 plane exchanged with rank `rank`."""
    _fields_ = [("rank", C.c_int32), ("send", C.c_uint32 * 4), ("recv", C.c_uint32 * 4)]


class Vertex(C.Structure):
    """pbr_vertex: VSInput_P3F_N3F_T2F_T2F, DeferredRendering/Shader/global.hlsli:59-66 (56 B)."""
    _fields_ = [("position", C.c_float * 3), ("normal", C.c_float * 3), ("tangent", C.c_float * 3), ("color", C.c_float * 3),
                ("uv", C.c_float * 2)]


class Draw(C.Structure):
    """pbr_draw: ConstantBufferInstance (gbuffer.hlsl:33-48) without the Use*Map flags, plus the draw's index range (164 B)."""
    _fields_ = [("Model", C.c_float * 16), ("InvModel", C.c_float * 16), ("Albedo", C.c_float * 3), ("Emission", C.c_float),
                ("Roughness", C.c_float), ("Metallic", C.c_float), ("first_index", C.c_uint32), ("index_count", C.c_uint32),
                ("base_vertex", C.c_int32)]


assert C.sizeof(Vertex) == 56 and C.sizeof(Draw) == 164
# the same records as numpy arrays (device uploads)
VERTEX_DTYPE = np.dtype([("position", np.float32, 3), ("normal", np.float32, 3), ("tangent", np.float32, 3),
                         ("color", np.float32, 3), ("uv", np.float32, 2)])
DRAW_DTYPE = np.dtype([("Model", np.float32, 16), ("InvModel", np.float32, 16), ("Albedo", np.float32, 3), ("Emission", np.float32),
                       ("Roughness", np.float32), ("Metallic", np.float32), ("first_index", np.uint32), ("index_count", np.uint32),
                       ("base_vertex", np.int32)])
assert VERTEX_DTYPE.itemsize == 56 and DRAW_DTYPE.itemsize == 164
# pbr_aabb: a draw's bound in its local (vertex) space, one per draw (an array parallel to the draws)
AABB_DTYPE = np.dtype([("min", np.float32, 3), ("max", np.float32, 3)])
assert AABB_DTYPE.itemsize == 24


class CullStats(C.Structure):
    """pbr_cull_stats: the reference's mCullingStatus (NumDrawCall, NumCulled) and the triangles either way (16 B)."""
    _fields_ = [("draws_drawn", C.c_uint32), ("draws_culled", C.c_uint32), ("triangles_drawn", C.c_uint32),
                ("triangles_culled", C.c_uint32)]

    def astuple(self):
        return (self.draws_drawn, self.draws_culled, self.triangles_drawn, self.triangles_culled)


assert C.sizeof(CullStats) == 16
RASTER_MAX_DRAWS = 65536                              # PBR_RASTER_MAX_DRAWS
RASTER_MAX_TRIANGLES = 1 << 22                        # PBR_RASTER_MAX_TRIANGLES
RASTER_MAX_SIZE = 8192                                # PBR_RASTER_MAX_SIZE


class Texture2D(C.Structure):
    """pbr_texture2d: a device mip chain in the reference's layout (level i (width >> i) x (height >> i), levels concatenated)
    and its DXGI format number (24 B); with TEX_BC1_BLOCKS in the format, the chain as BC1 blocks (texture2d_bytes)."""
    _fields_ = [("texels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("mip_levels", C.c_uint32),
                ("format", C.c_uint32)]


assert C.sizeof(Texture2D) == 24
# pbr_draw_maps: per draw, the texture index of each map, NO_MAP = the constant branch (an array parallel to the draws)
DRAW_MAPS_DTYPE = np.dtype([("albedo", np.uint32), ("normal", np.uint32), ("roughness", np.uint32), ("metallic", np.uint32),
                            ("ao", np.uint32)])
assert DRAW_MAPS_DTYPE.itemsize == 20
MAP_NAMES = DRAW_MAPS_DTYPE.names
NO_MAP = 0xFFFFFFFF                                   # PBR_NO_MAP
RASTER_MAX_TEXTURES = 64                              # PBR_RASTER_MAX_TEXTURES
TEX_MAX_SIZE = 16384                                  # PBR_TEX_MAX_SIZE
# DXGI formats the textured raster reads (PBR_TEX_*): number -> (bytes per texel, sRGB)
TEX_R8G8B8A8_UNORM, TEX_B8G8R8A8_UNORM, TEX_B8G8R8A8_UNORM_SRGB, TEX_R8_UNORM = 28, 87, 91, 61
TEX_FORMATS = {TEX_R8G8B8A8_UNORM: (4, False), TEX_B8G8R8A8_UNORM: (4, False), TEX_B8G8R8A8_UNORM_SRGB: (4, True),
               TEX_R8_UNORM: (1, False)}
TEX_BC1_BLOCKS = 0x100                                # PBR_TEX_BC1_BLOCKS: ORed into a format, the chain is held as BC1 blocks


def texture2d_bytes(width, height, mip_levels, fmt):
    """pbr_texture2d_bytes: the bytes of a whole chain, decoded (level i (width >> i) x (height >> i) texels) or, with
    TEX_BC1_BLOCKS in fmt, BC1 (level i max(1, ((width >> i) + 3) // 4) x max(1, ((height >> i) + 3) // 4) blocks of 8 bytes);
    0 for a description the library refuses."""
    width, height, mip_levels, fmt = int(width), int(height), int(mip_levels), int(fmt)
    if fmt & ~(0xFF | TEX_BC1_BLOCKS) or (fmt & 0xFF) not in TEX_FORMATS:
        return 0
    if not (1 <= width <= TEX_MAX_SIZE and 1 <= height <= TEX_MAX_SIZE and 1 <= mip_levels <= min(width, height).bit_length()):
        return 0
    if fmt & TEX_BC1_BLOCKS:
        return sum(max(1, ((width >> l) + 3) // 4) * max(1, ((height >> l) + 3) // 4) * 8 for l in range(mip_levels))
    return sum((width >> l) * (height >> l) for l in range(mip_levels)) * TEX_FORMATS[fmt][0]


BC6H_MAX_SIZE = 8192                                  # PBR_BC6H_MAX_SIZE


BC6H_ENCODE_TWO_REGION = 1     # PBR_BC6H_ENCODE_TWO_REGION: pbr_bc6h_encode_cube_ex may use the ten two-region modes as well


def bc6h_chain_bytes(size, mip_levels):
    """pbr_bc6h_chain_bytes: the bytes of one cube face's mip chain as BC6H blocks (level i max(1, ((size >> i) + 3) // 4)^2 blocks
    of 16 bytes); 0 for what pbr_bc6h_decode_cube refuses (size 0, not a multiple of 4 or above BC6H_MAX_SIZE, mip_levels 0 or
    above floor(log2(size)) + 1)."""
    size, mip_levels = int(size), int(mip_levels)
    if not (4 <= size <= BC6H_MAX_SIZE) or size % 4 or not (1 <= mip_levels <= size.bit_length()):
        return 0
    return sum(max(1, ((size >> l) + 3) // 4) ** 2 * 16 for l in range(mip_levels))


EQUIRECT_MAX_W, EQUIRECT_MAX_H = 16384, 8192          # PBR_EQUIRECT_MAX_W / _H
EQUIRECT_SRC_RGBE = 1          # PBR_EQUIRECT_SRC_RGBE: the panorama is Radiance RGBE texels (4 bytes), decoded where they are fetched


def equirect_default_size(pw):
    """pbr_equirect_default_size: the cube size an import picks for a panorama pw texels wide — the largest power of two <= pw / 4
    (a face spans a quarter of the width), clamped to [4, BC6H_MAX_SIZE]"""
    q = int(pw) // 4
    return min(max(1 << (q.bit_length() - 1) if q else 0, 4), BC6H_MAX_SIZE)


def equirect_default_samples(pw, size):
    """pbr_equirect_default_samples: the smallest of 1, 2, 4, 8 with 4 size samples >= pw, and 8 if none is"""
    return next((s for s in (1, 2, 4) if 4 * int(size) * s >= int(pw)), 8)


class CubeF32(C.Structure):
    _fields_ = [("data", C.c_void_p), ("size", C.c_uint32), ("mips", C.c_uint32)]


class CubeBc6h(C.Structure):                          # pbr_cube_bc6h: six DEVICE pointers to BC6H_UF16 chains, order px .. nz
    _fields_ = [("face_blocks", C.c_void_p * 6), ("size", C.c_uint32), ("mips", C.c_uint32)]


# PointLight, DeferredPipeline.h:341-347 (44 B)
LIGHT_DTYPE = np.dtype([
    ("Position", np.float32, 3), ("Color", np.float32, 3), ("Intensity", np.float32),
    ("Radius", np.float32), ("C0", np.float32), ("C1", np.float32), ("C2", np.float32),
])
assert LIGHT_DTYPE.itemsize == 44

# Cluster, DeferredPipeline.h:333-339 (156 B)
CLUSTER_DTYPE = np.dtype([
    ("MinBound", np.float32, 3), ("MaxBound", np.float32, 3), ("NumLights", np.int32),
    ("LightIndex", np.int32, MAX_LIGHTS_PER_CLUSTER),
])
assert CLUSTER_DTYPE.itemsize == 156


def cube_mip_offset(size: int, mip: int) -> int:
    """Texel offset of mip `mip` in a cube chain (mips concatenated, 6 faces per mip)."""
    return sum(6 * (size >> m) ** 2 for m in range(mip))


def cube_texels(size: int, mips: int) -> int:
    return cube_mip_offset(size, mips)


def env_padded_mip_offset(size: int, mip: int) -> int:
    """Texel offset of mip `mip` in the footprint layout of pbr_env_pad (4 texels per bilinear footprint origin,
    (s+1)^2 origins per face)."""
    return sum(6 * ((size >> m) + 1) ** 2 * 4 for m in range(mip))


def env_padded_texels(size: int, mips: int) -> int:
    return env_padded_mip_offset(size, mips)


def bloom_level_offset(w: int, h: int, level: int) -> int:
    return sum((w >> l) * (h >> l) for l in range(level))


def bloom_chain_texels(w: int, h: int) -> int:
    return bloom_level_offset(w, h, BLOOM_MIPS)
