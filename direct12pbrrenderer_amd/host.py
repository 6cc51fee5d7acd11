"""ctypes binding of libpbr_host.so (direct12pbrrenderer_amd/host/pbr_host.h): the C++ pass graph — RenderScheduler ->
FrameGraph -> the reference-shaped pass classes -> HipCommandList -> the C ABI of include/pbr_hip.h.

This is the drop-in side of the boundary: a host program written against the reference's pass API runs the HIP
kernels through it.  Python only loads the library and hands over host arrays; nothing here computes."""
import ctypes as C
import os

import numpy as np

from .structs import BC6H_ENCODE_TWO_REGION

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpbr_host.so")
_u32, _vp, _int = C.c_uint32, C.c_void_p, C.c_int

SIGNATURES = {
    "pbrh_create": (_vp, [_int, _u32, _u32, _u32, _u32, C.c_char_p, C.c_size_t]),
    "pbrh_create_tile": (_vp, [_int, _u32, _u32, _u32, _u32, _u32, _int, _u32, _u32, C.c_char_p, C.c_size_t]),
    "pbrh_tile_layout": (_int, [_u32, _u32, _u32, _u32, _u32, _int, _vp, _vp, _int]),
    "pbrh_destroy": (None, [_vp]),
    "pbrh_last_error": (C.c_char_p, [_vp]),
    "pbrh_set_skybox": (_int, [_vp, _vp, _u32]),
    "pbrh_load_skybox": (_int, [_vp, C.c_char_p]),
    "pbrh_set_lights": (_int, [_vp, _vp, _int]),
    "pbrh_load_scene_lights": (_int, [_vp, C.c_char_p]),
    "pbrh_parse_scene_lights": (_int, [C.c_char_p, C.c_size_t, _vp, _int, C.c_char_p, C.c_size_t]),
    "pbrh_light_buffer": (_int, [_u32, _u32, _vp, _vp, _int, _vp, _int]),
    "pbrh_set_gbuffer": (_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "pbrh_set_materials": (_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "pbrh_set_meshes": (_int, [_vp, _vp, _u32, _vp, _u32, _vp, _u32]),
    "pbrh_set_textured_meshes": (_int, [_vp, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _u32]),
    "pbrh_set_model_culling": (_int, [_vp, _int]),
    "pbrh_culling_status": (_int, [_vp, C.POINTER(_u32 * 4)]),
    "pbrh_set_initial_luminance": (_int, [_vp, C.c_float]),
    "pbrh_set_tile": (_int, [_vp] + [_u32] * 8),
    "pbrh_comm_init": (_int, [_vp, _int, _int, _vp]),
    "pbrh_set_halo_loopback": (_int, [_vp, _int]),
    "pbrh_halo_copy_from": (_int, [_vp, _vp]),
    "pbrh_set_frames_in_flight": (_int, [_vp, _int]),
    "pbrh_set_tail_overlap": (_int, [_vp, _int]),
    "pbrh_set_external_histogram": (_int, [_vp, _vp]),
    "pbrh_capture_histogram": (_int, [_vp, _int]),
    "pbrh_captured_histogram": (_int, [_vp, _vp]),
    "pbrh_set_fused": (_int, [_vp, _int]),
    "pbrh_set_antialiasing": (_int, [_vp, _int]),
    "pbrh_presented": (_int, [_vp, C.c_char_p, C.c_size_t]),
    "pbrh_set_sun_light": (_int, [_vp, C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 3), C.c_uint32, C.c_uint32, C.c_float, C.c_float, _int]),
    "pbrh_clear_sun_light": (_int, [_vp]),
    "pbrh_set_sun_shadow_depth_only": (_int, [_vp, _int]),
    "pbrh_render_n": (_int, [_vp, _int, C.c_float, C.POINTER(C.c_double)]),
    "pbrh_render": (_int, [_vp, C.c_float]),
    "pbrh_execution_order": (_int, [_vp, C.c_char_p, C.c_size_t]),
    "pbrh_dispatch_count": (_int, [_vp]),
    "pbrh_event_log": (_int, [_vp, C.c_char_p, C.c_size_t]),
    "pbrh_read": (C.c_long, [_vp, C.c_char_p, _vp, C.c_size_t]),
    "pbrh_get_global": (_int, [_vp, _vp]),
    "pbrh_cull_lights": (_int, [_u32, _u32, _vp, _vp, _int, _vp, _int]),
    "pbrh_scene_light_bounds": (_int, [_u32, _u32, _vp, C.c_char_p, C.c_size_t, _vp, _int, _vp, _vp, C.c_char_p, C.c_size_t]),
    "pbrh_dry_run_execution_order": (_int, [_u32, _u32, C.c_char_p, C.c_size_t]),
    "pbrh_probe_binding": (_int, [C.c_char_p, _int, C.c_char_p, _int]),
    "pbrh_parse_hdr": (_int, [_vp, C.c_size_t, _vp, _vp, _vp, C.c_size_t, C.c_char_p, C.c_size_t]),
    "pbrh_parse_texture_file": (_int, [_vp, C.c_size_t, _vp, _vp, C.c_size_t, C.c_char_p, C.c_size_t]),
    "pbrh_write_texture_file": (C.c_long, [_vp, _vp, C.c_size_t, C.c_char_p, C.c_size_t]),
    "pbrh_parse_cubemap_file": (_int, [_vp, C.c_size_t, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(C.c_size_t * 6), _vp, C.c_char_p, C.c_size_t]),
    "pbrh_write_cubemap_file": (C.c_long, [C.POINTER(_vp * 6), _u32, _u32, _u32, _vp, _vp, C.c_size_t, C.c_char_p, C.c_size_t]),
    "pbrh_set_skybox_file": (_int, [_vp, _vp, C.c_size_t, _int]),
    "pbrh_load_skybox_file": (_int, [_vp, C.c_char_p, _int]),
    "pbrh_set_skybox_file_resident": (_int, [_vp, _vp, C.c_size_t, _int]),
    "pbrh_load_skybox_file_resident": (_int, [_vp, C.c_char_p, _int]),
    "pbrh_sky_resident_bytes": (C.c_size_t, [_vp]),
    "pbrh_import_texture": (C.c_long, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, C.c_size_t, C.c_char_p, C.c_size_t]),
    "pbrh_import_cubemap": (C.c_long, [_vp, _vp, _u32, _u32, _vp, C.c_size_t, C.c_char_p, C.c_size_t]),
    "pbrh_import_cubemap_dir": (C.c_long, [_vp, C.c_char_p, _u32, _vp, C.c_size_t, C.c_char_p, C.c_size_t]),
    "pbrh_import_cubemap_ex": (C.c_long, [_vp, _vp, _u32, _u32, _u32, _vp, C.c_size_t, C.c_char_p, C.c_size_t]),
    "pbrh_import_cubemap_dir_ex": (C.c_long, [_vp, C.c_char_p, _u32, _u32, _vp, C.c_size_t, C.c_char_p, C.c_size_t]),
    "pbrh_import_cubemap_equirect": (C.c_long, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, C.c_size_t, C.c_char_p, C.c_size_t]),
    "pbrh_import_cubemap_hdr": (C.c_long, [_vp, C.c_char_p, _u32, _u32, _u32, _u32, _vp, C.c_size_t, C.c_char_p, C.c_size_t]),
    "pbrh_load_skybox_equirect": (_int, [_vp, C.c_char_p, _u32, _u32]),
}

_lib = None


def load():
    """dlopen libpbr_host.so (after torch: one HIP runtime per process, see _lib.load) and type every entry point."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: build it with `make -C direct12pbrrenderer_amd/host` (or __graft_entry__.build())")
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class HostError(RuntimeError):
    pass


def pack_lights(lights):
    """structured light array (structs.LIGHT_DTYPE) -> the 8-float records pbrh_set_lights takes: position, colour, radius, intensity."""
    n = len(lights)
    return np.ascontiguousarray(np.concatenate([lights["Position"], lights["Color"], lights["Radius"].reshape(n, 1),
                                                lights["Intensity"].reshape(n, 1)], axis=1).astype(np.float32))


def parse_texture_file(data):
    """One of the reference's serialized textures (the bytes of a texture asset's _data.bin) -> (blocks, width, height, mip_levels,
    format): the chain's BC1 blocks (uint8) and its description with format = the stored format | structs.TEX_BC1_BLOCKS, as
    PbrContext.upload_texture and HostRenderer.set_textured_meshes take them.  No decode happens on the CPU."""
    from .structs import Texture2D
    lib = load()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    err = C.create_string_buffer(256)
    t = Texture2D()
    if lib.pbrh_parse_texture_file(buf.ctypes.data, buf.size, C.addressof(t), None, 0, err, 256) != 0:
        raise HostError(err.value.decode())
    blocks = np.zeros(buf.size - 16, dtype=np.uint8)
    if lib.pbrh_parse_texture_file(buf.ctypes.data, buf.size, C.addressof(t), blocks.ctypes.data, blocks.size, err, 256) != 0:
        raise HostError(err.value.decode())
    return blocks, t.width, t.height, t.mip_levels, t.format


def write_texture_file(blocks, width, height, mip_levels, fmt):
    """The inverse of parse_texture_file: a BC1 chain (uint8 blocks) and its description (fmt = the stored format |
    structs.TEX_BC1_BLOCKS) -> the bytes of the reference's serialized texture (TextureInfo, byte count, payload)."""
    from .structs import Texture2D, texture2d_bytes
    lib = load()
    blocks = np.ascontiguousarray(blocks).view(np.uint8).reshape(-1)
    err = C.create_string_buffer(256)
    t = Texture2D(blocks.ctypes.data, int(width), int(height), int(mip_levels), int(fmt))
    need = lib.pbrh_write_texture_file(C.addressof(t), None, 0, err, 256)
    if need < 0:
        raise HostError(err.value.decode())
    if blocks.size != texture2d_bytes(width, height, mip_levels, fmt):
        raise HostError(f"texture file: {blocks.size} block bytes, the description takes {need - 16}")
    out = np.zeros(need, dtype=np.uint8)
    if lib.pbrh_write_texture_file(C.addressof(t), out.ctypes.data, out.size, err, 256) != need:
        raise HostError(err.value.decode())
    return out.tobytes()


def parse_cubemap_file(data):
    """One of the reference's serialized sky cubes (the bytes of a CubeMapResource's data file) -> (size, mip_levels, face_offsets,
    sh_pack): the byte offset of each face's BC6H_UF16 chain in the file (six ints, each a multiple of 16; a face holds
    structs.bc6h_chain_bytes(size, mip_levels) bytes; order px, nx, py, ny, pz, nz) and the file's SH2CoefficientsPack as 28 floats.
    No decode happens on the CPU: upload the file and hand PbrContext.bc6h_decode_cube the six addresses."""
    lib = load()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    err = C.create_string_buffer(256)
    size, mips, offsets, sh = _u32(0), _u32(0), (C.c_size_t * 6)(), np.zeros(28, np.float32)
    if lib.pbrh_parse_cubemap_file(buf.ctypes.data if buf.size else None, buf.size, C.byref(size), C.byref(mips), C.byref(offsets),
                                   sh.ctypes.data, err, 256) != 0:
        raise HostError(err.value.decode())
    return int(size.value), int(mips.value), [int(o) for o in offsets], sh


def write_cubemap_file(faces, size, mip_levels, sh_pack, fmt=2):
    """The inverse of parse_cubemap_file: six face chains of BC6H blocks (uint8, structs.bc6h_chain_bytes(size, mip_levels) each) and
    the 28 floats of the SH pack -> the bytes of the reference's serialized sky cube.  fmt: the DXGI number written into every
    TextureInfo, one of the reference's HDR formats (1 .. 18; 2 = R32G32B32A32_FLOAT, what its sky import produces)."""
    from .structs import bc6h_chain_bytes
    lib = load()
    faces = [np.ascontiguousarray(f).view(np.uint8).reshape(-1) for f in faces]
    if len(faces) != 6:
        raise HostError(f"cube-map file: six faces, got {len(faces)}")
    sh = np.ascontiguousarray(sh_pack, dtype=np.float32).reshape(-1)
    if sh.size != 28:
        raise HostError(f"cube-map file: the SH pack is 28 floats, got {sh.size}")
    err = C.create_string_buffer(256)
    ptrs = (_vp * 6)(*[f.ctypes.data for f in faces])
    need = lib.pbrh_write_cubemap_file(C.byref(ptrs), int(size), int(mip_levels), int(fmt), sh.ctypes.data, None, 0, err, 256)
    if need < 0:
        raise HostError(err.value.decode())
    for f in faces:
        if f.size != bc6h_chain_bytes(size, mip_levels):
            raise HostError(f"cube-map file: a face of {f.size} bytes, the description takes {bc6h_chain_bytes(size, mip_levels)}")
    out = np.zeros(need, dtype=np.uint8)
    if lib.pbrh_write_cubemap_file(C.byref(ptrs), int(size), int(mip_levels), int(fmt), sh.ctypes.data, out.ctypes.data, out.size, err, 256) != need:
        raise HostError(err.value.decode())
    return out.tobytes()


class HostRenderer:
    """One DeferredRenderPipeline + FrameGraph + RenderScheduler (pbrh_renderer).  tile = (full_w, full_h, cols, rows, rank,
    halo) renders one device's tile of a larger frame; otherwise a whole width x height frame."""

    def __init__(self, device, width=None, height=None, env_size=512, lut_res=512, tile=None):
        self.lib = load()
        err = C.create_string_buffer(512)
        if tile is not None:
            fw, fh, cols, rows, rank, halo = tile
            self.h = self.lib.pbrh_create_tile(int(device), fw, fh, cols, rows, rank, 1 if halo else 0, env_size, lut_res, err, 512)
        else:
            self.h = self.lib.pbrh_create(int(device), width, height, env_size, lut_res, err, 512)
        if not self.h:
            raise HostError(f"pbrh_create failed: {err.value.decode()}")

    def _check(self, st):
        if st != 0:
            raise HostError(self.lib.pbrh_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.pbrh_destroy(self.h)
            self.h = None

    def set_skybox(self, cube_mip0, size):
        a = np.ascontiguousarray(cube_mip0[:4 * 6 * size * size], dtype=np.float32)
        self._check(self.lib.pbrh_set_skybox(self.h, a.ctypes.data, size))

    def set_skybox_file(self, data, recompute_sh=False, resident=False):
        """pbrh_set_skybox_file: the bytes of the reference's serialized sky cube are uploaded as they are and decoded on the GPU
        (pbr_bc6h_decode_cube) with the file's own levels; SkyBoxSH is the file's pack, or with recompute_sh the projection of the
        decoded level 0.  resident (pbrh_set_skybox_file_resident): the uploaded file stays the renderer's sky and the sky pass
        samples its BC6H blocks in place — the same frames at 1 byte per sky texel instead of 16."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        fn = self.lib.pbrh_set_skybox_file_resident if resident else self.lib.pbrh_set_skybox_file
        self._check(fn(self.h, buf.ctypes.data if buf.size else None, buf.size, 1 if recompute_sh else 0))

    def load_skybox_file(self, path, recompute_sh=False, resident=False):
        """set_skybox_file of a file on disk (pbrh_load_skybox_file / pbrh_load_skybox_file_resident)"""
        fn = self.lib.pbrh_load_skybox_file_resident if resident else self.lib.pbrh_load_skybox_file
        self._check(fn(self.h, os.fsencode(path), 1 if recompute_sh else 0))

    def sky_resident_bytes(self):
        """pbrh_sky_resident_bytes: the device bytes the renderer holds for its sky (the decoded cube's or the resident file's)"""
        return int(self.lib.pbrh_sky_resident_bytes(self.h))

    def set_lights(self, lights):
        p = pack_lights(lights)
        self._check(self.lib.pbrh_set_lights(self.h, p.ctypes.data, len(p)))

    def load_scene_lights(self, path):
        """the mSceneLight records of a reference scene file (Asset/Scene/main.json) become the renderer's lights"""
        self._check(self.lib.pbrh_load_scene_lights(self.h, os.fsencode(path)))

    def set_gbuffer(self, gb):
        planes = [np.ascontiguousarray(gb[k]) for k in ("A", "B", "C", "depth", "stencil")]
        self._check(self.lib.pbrh_set_gbuffer(self.h, *[p.ctypes.data for p in planes]))

    def set_meshes(self, vertices, indices, draws):
        """constant-material meshes (structs.VERTEX_DTYPE, uint32 indices, structs.DRAW_DTYPE records): GBufferPass rasterizes them
        every frame (pbr_gbuffer_raster) instead of uploading planes"""
        from .structs import DRAW_DTYPE, VERTEX_DTYPE
        v = np.ascontiguousarray(vertices, dtype=VERTEX_DTYPE)
        i = np.ascontiguousarray(indices, dtype=np.uint32)
        d = np.ascontiguousarray(draws, dtype=DRAW_DTYPE)
        self._check(self.lib.pbrh_set_meshes(self.h, v.ctypes.data, len(v), i.ctypes.data, len(i), d.ctypes.data, len(d)))

    def set_textured_meshes(self, vertices, indices, draws, maps, textures):
        """set_meshes plus the draws' maps (structs.DRAW_MAPS_DTYPE, one per draw) and their textures: (chain, width, height,
        mip_levels, format) with the chain's host bytes in the reference's layout (scene.pack_chain) or, with structs.TEX_BC1_BLOCKS
        in the format, its BC1 blocks (parse_texture_file), which stay BC1 on the device.  GBufferPass uploads the chains once and
        rasterizes through pbr_gbuffer_raster with maps."""
        from .structs import DRAW_DTYPE, DRAW_MAPS_DTYPE, VERTEX_DTYPE, Texture2D
        v = np.ascontiguousarray(vertices, dtype=VERTEX_DTYPE)
        i = np.ascontiguousarray(indices, dtype=np.uint32)
        d = np.ascontiguousarray(draws, dtype=DRAW_DTYPE)
        m = np.ascontiguousarray(maps, dtype=DRAW_MAPS_DTYPE)
        chains = [np.ascontiguousarray(t[0]).view(np.uint8) for t in textures]
        table = (Texture2D * max(len(chains), 1))(*[Texture2D(c.ctypes.data, int(t[1]), int(t[2]), int(t[3]), int(t[4]))
                                                   for c, t in zip(chains, textures)])
        self._check(self.lib.pbrh_set_textured_meshes(self.h, v.ctypes.data, len(v), i.ctypes.data, len(i), d.ctypes.data, len(d),
                                                      m.ctypes.data, C.addressof(table), len(chains)))

    def set_model_culling(self, on=True):
        """pbrh_set_model_culling: GBufferPass culls the meshes' draws against the frustum on the device (the reference's
        Scene::CullModel; bounds made on the GPU at upload).  The frame is bit-identical; default off."""
        self._check(self.lib.pbrh_set_model_culling(self.h, 1 if on else 0))

    def culling_status(self):
        """pbrh_culling_status: (draws drawn, draws culled, triangles drawn, triangles culled) of the last frame rendered with
        culling on — the reference's mCullingStatus; synchronises"""
        out = (C.c_uint32 * 4)()
        self._check(self.lib.pbrh_culling_status(self.h, C.byref(out)))
        return tuple(int(x) for x in out)

    def import_texture(self, level0, fmt, mip_levels=None):
        """pbrh_import_texture: host level 0 (uint8 [h, w] for R8, [h, w, 4] otherwise; sizes multiples of 4) -> the bytes of the
        reference's texture file holding its whole mip chain (all levels by default) as BC1 blocks, made on the GPU."""
        lv0 = np.ascontiguousarray(level0, dtype=np.uint8)
        if lv0.ndim != (2 if int(fmt) == 61 else 3) or (lv0.ndim == 3 and lv0.shape[2] != 4):
            raise HostError(f"import_texture: level 0 of format {fmt} has shape {lv0.shape}")
        h, w = lv0.shape[:2]
        mips = min(w, h).bit_length() if mip_levels is None else int(mip_levels)
        err = C.create_string_buffer(256)
        need = self.lib.pbrh_import_texture(self.h, None, w, h, int(fmt), mips, None, 0, err, 256)
        if need < 0:
            raise HostError(err.value.decode())
        out = np.zeros(need, dtype=np.uint8)
        if self.lib.pbrh_import_texture(self.h, lv0.ctypes.data, w, h, int(fmt), mips, out.ctypes.data, out.size, err, 256) != need:
            raise HostError(err.value.decode())
        return out.tobytes()

    def import_cubemap(self, level0, mip_levels=None, two_region=False):
        """pbrh_import_cubemap_ex: host level 0 of a sky (float32 [6, size, size, 4] or the flat equivalent, faces px, nx, py, ny, pz, nz)
        -> the bytes of the reference's serialized sky cube: box mips, the SH pack of the fp32 level 0 and the BC6H_UF16 chains (all
        levels by default), made on the GPU.  set_skybox_file and DeferredFrame.set_sky_file take them as they are.  two_region: the
        compression may use the ten two-region modes as well (PBR_BC6H_ENCODE_TWO_REGION); the file is read like any other."""
        lv0 = np.ascontiguousarray(level0, dtype=np.float32).reshape(-1, 4)
        size = int(round((len(lv0) // 6) ** 0.5))
        if 6 * size * size != len(lv0):
            raise HostError(f"import_cubemap: level 0 of {len(lv0)} texels is not six square faces")
        mips, flags = 0 if mip_levels is None else int(mip_levels), BC6H_ENCODE_TWO_REGION if two_region else 0
        err = C.create_string_buffer(256)
        need = self.lib.pbrh_import_cubemap_ex(self.h, None, size, mips, flags, None, 0, err, 256)
        if need < 0:
            raise HostError(err.value.decode())
        out = np.zeros(need, dtype=np.uint8)
        if self.lib.pbrh_import_cubemap_ex(self.h, lv0.ctypes.data, size, mips, flags, out.ctypes.data, out.size, err, 256) != need:
            raise HostError(err.value.decode())
        return out.tobytes()

    def import_cubemap_dir(self, path, mip_levels=None, two_region=False):
        """pbrh_import_cubemap_dir_ex: import_cubemap of <path>/{px,nx,py,ny,pz,nz}.hdr (load_skybox's parse, RGBE expanded on the GPU)"""
        mips, flags = 0 if mip_levels is None else int(mip_levels), BC6H_ENCODE_TWO_REGION if two_region else 0
        err = C.create_string_buffer(256)
        need = self.lib.pbrh_import_cubemap_dir_ex(self.h, os.fsencode(path), mips, flags, None, 0, err, 256)
        if need < 0:
            raise HostError(err.value.decode())
        out = np.zeros(need, dtype=np.uint8)
        if self.lib.pbrh_import_cubemap_dir_ex(self.h, os.fsencode(path), mips, flags, out.ctypes.data, out.size, err, 256) != need:
            raise HostError(err.value.decode())
        return out.tobytes()

    def import_cubemap_equirect(self, pano, size=None, samples=None, mip_levels=None, two_region=False):
        """pbrh_import_cubemap_equirect: import_cubemap of ONE equirectangular panorama (host float32 [ph, pw, 4], row 0 the top),
        resampled into level 0 on the GPU (PbrContext.equirect_to_cube's rule) at `size` with samples^2 sub-samples a texel; None for
        either: the default rule (structs.equirect_default_size / equirect_default_samples)."""
        p = np.ascontiguousarray(pano, dtype=np.float32)
        if p.ndim != 3 or p.shape[2] != 4:
            raise HostError(f"import_cubemap_equirect: a panorama is float32 [ph, pw, 4], got {p.shape}")
        ph, pw = p.shape[:2]
        args = (pw, ph, int(size or 0), int(samples or 0), 0 if mip_levels is None else int(mip_levels), BC6H_ENCODE_TWO_REGION if two_region else 0)
        err = C.create_string_buffer(256)
        need = self.lib.pbrh_import_cubemap_equirect(self.h, None, *args, None, 0, err, 256)
        if need < 0:
            raise HostError(err.value.decode())
        out = np.zeros(need, dtype=np.uint8)
        if self.lib.pbrh_import_cubemap_equirect(self.h, p.ctypes.data, *args, out.ctypes.data, out.size, err, 256) != need:
            raise HostError(err.value.decode())
        return out.tobytes()

    def import_cubemap_hdr(self, path, size=None, samples=None, mip_levels=None, two_region=False):
        """pbrh_import_cubemap_hdr: import_cubemap_equirect of one Radiance .hdr file of any aspect ratio; its RGBE texels are uploaded
        as they are and decoded where the kernel fetches them"""
        args = (int(size or 0), int(samples or 0), 0 if mip_levels is None else int(mip_levels), BC6H_ENCODE_TWO_REGION if two_region else 0)
        err = C.create_string_buffer(256)
        need = self.lib.pbrh_import_cubemap_hdr(self.h, os.fsencode(path), *args, None, 0, err, 256)
        if need < 0:
            raise HostError(err.value.decode())
        out = np.zeros(need, dtype=np.uint8)
        if self.lib.pbrh_import_cubemap_hdr(self.h, os.fsencode(path), *args, out.ctypes.data, out.size, err, 256) != need:
            raise HostError(err.value.decode())
        return out.tobytes()

    def load_skybox_equirect(self, path, size=None, samples=None):
        """pbrh_load_skybox_equirect: load_skybox for one equirectangular .hdr — the fp32 sky with box mips and SH9, level 0 resampled
        from the file's RGBE texels on the GPU; None: the default rule for the size / the sub-sample count"""
        self._check(self.lib.pbrh_load_skybox_equirect(self.h, os.fsencode(path), int(size or 0), int(samples or 0)))

    def set_initial_luminance(self, v):
        self._check(self.lib.pbrh_set_initial_luminance(self.h, float(v)))

    def set_fused(self, on):
        self._check(self.lib.pbrh_set_fused(self.h, 1 if on else 0))

    def set_antialiasing(self, on=True):
        """pbrh_set_antialiasing: AntiAliasPass (the integer edge filter pbr_fxaa) between ToneMapping and Present.  It writes the
        texture "AntiAliasedTexture" (read(name, (h, w), np.uint32)), which becomes the presented one; "ToneMappedTexture" stays
        what it is.  Off by default.  A tile renderer and one with an overlapped tail refuse (HostError)."""
        self._check(self.lib.pbrh_set_antialiasing(self.h, 1 if on else 0))

    def set_sun_light(self, direction, luminance=100.0, map_size=2048, pcf=3, bias=(5e-4, 4e-3), shadows=True, depth_only=False):
        """pbrh_set_sun_light: SunLightPass (pbr_sun_light) between DeferredShading and Bloom and, with shadows, SunShadowPass after
        GBuffer (needs set_meshes; the map is the frame-graph texture "SunShadowDepth", rasterized once per mesh upload / call).
        direction None: pbrh_clear_sun_light.  The arguments are DeferredFrame.set_sun's; tiles and an overlapped tail refuse.
        depth_only (pbrh_set_sun_shadow_depth_only): SunShadowPass makes the same map with pbr_depth_raster, still in one dispatch,
        without the map-sized scratch planes."""
        if direction is None:
            self._check(self.lib.pbrh_clear_sun_light(self.h))
            return
        self._check(self.lib.pbrh_set_sun_shadow_depth_only(self.h, 1 if depth_only else 0))
        lum = np.broadcast_to(np.asarray(luminance, dtype=np.float32), (3,))
        self._check(self.lib.pbrh_set_sun_light(self.h, C.byref((C.c_float * 3)(*[float(v) for v in direction])),
                                                C.byref((C.c_float * 3)(*[float(v) for v in lum])), int(map_size), int(pcf), float(bias[0]),
                                                float(bias[1]), 1 if shadows else 0))

    def presented(self):
        """the name of the frame-graph texture the present pass shows"""
        buf = C.create_string_buffer(128)
        self._check(self.lib.pbrh_presented(self.h, buf, 128))
        return buf.value.decode()

    def set_frames_in_flight(self, k):
        self._check(self.lib.pbrh_set_frames_in_flight(self.h, int(k)))

    def set_tail_overlap(self, on):
        """0 / False: off; 1 / True: from the average-luminance dispatch; 2: from the bloom pass (frames without a halo exchange)"""
        self._check(self.lib.pbrh_set_tail_overlap(self.h, int(on)))

    def comm_init(self, world, rank, unique_id):
        buf = C.create_string_buffer(unique_id, 128) if unique_id is not None else None
        self._check(self.lib.pbrh_comm_init(self.h, world, rank, C.cast(buf, C.c_void_p) if buf else None))

    def set_halo_loopback(self, on):
        """halo mode without a communicator: the exchange packs / unpacks the staging area and moves nothing (tests and the one-GPU
        rehearsal of bench.py, which carry the strips — or nothing — themselves)"""
        self._check(self.lib.pbrh_set_halo_loopback(self.h, 1 if on else 0))

    def capture_histogram(self, on):
        self._check(self.lib.pbrh_capture_histogram(self.h, 1 if on else 0))

    def captured_histogram(self):
        """the tile's own 256 luminance counts of the last frame rendered with capture_histogram(True)"""
        h = np.zeros(256, dtype=np.uint32)
        self._check(self.lib.pbrh_captured_histogram(self.h, h.ctypes.data))
        return h

    def set_external_histogram(self, counts256):
        """counts of the OTHER tiles, added before the average (what pbr_allreduce_hist does over RCCL); None: none"""
        if counts256 is None:
            self._check(self.lib.pbrh_set_external_histogram(self.h, None))
        else:
            c = np.ascontiguousarray(counts256, dtype=np.uint32)
            assert c.size == 256
            self._check(self.lib.pbrh_set_external_histogram(self.h, c.ctypes.data))

    def render(self, dt=1.0 / 60.0):
        self._check(self.lib.pbrh_render(self.h, dt))

    def render_n(self, n, dt=1.0 / 60.0):
        """n frames; returns the average wall time per frame in ms (the queue is drained before the clock stops)."""
        ms = C.c_double(0.0)
        self._check(self.lib.pbrh_render_n(self.h, int(n), dt, C.byref(ms)))
        return ms.value

    def dispatch_count(self):
        return int(self.lib.pbrh_dispatch_count(self.h))

    def read(self, name, shape, dtype):
        a = np.zeros(shape, dtype=dtype)
        n = self.lib.pbrh_read(self.h, name.encode(), a.ctypes.data, a.nbytes)
        if n != a.nbytes:
            raise HostError(f"pbrh_read({name}): {n} of {a.nbytes} bytes: {self.lib.pbrh_last_error(self.h).decode()}")
        return a
