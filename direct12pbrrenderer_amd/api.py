"""Thin Python host wrapper over the C ABI (include/pbr_hip.h).

PyTorch is used only as plumbing: device allocations (torch tensors), the current HIP stream
and torch.distributed.  Every method below is one C-ABI call on device pointers; errors raise
RuntimeError with pbr_last_error(), mirroring the reference's throw-on-failure
(ThrowIfFailed, Engine/Include/Renderer/Device/Direct12/D3DUtils.h:12-41).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .structs import (Aabb, BloomDesc, BloomPrefilterDesc, DepthRasterDesc, RasterDesc, ShadeDesc, ShadeTables, Sun, SunDesc, Texture2D, BLOOM_KNEE, BLOOM_THRESHOLD, CLUSTER_DTYPE, ENV_MIPS, HISTOGRAM_BINS,
                      INV_LOG_LUMINANCE_RANGE, LIGHT_DTYPE, LOG_LUMINANCE_RANGE, MIN_LOG_LUMINANCE,
                      NUM_CLUSTERS, AABB_DTYPE, CullStats, DRAW_DTYPE, DRAW_MAPS_DTYPE, BC6H_ENCODE_TWO_REGION, BC6H_MAX_SIZE, EQUIRECT_SRC_RGBE, TEX_BC1_BLOCKS, TEX_FORMATS, VERTEX_DTYPE, CubeBc6h, CubeF32, FxaaImage, GBuffer, Global, HaloPeer, Tile, View, bloom_chain_texels, bc6h_chain_bytes, cube_texels, env_padded_texels, equirect_default_samples, equirect_default_size, texture2d_bytes)


class PbrError(RuntimeError):
    pass


LAUNCH_LOG = 64   # PBR_LAUNCH_LOG (include/pbr_hip.h): the launches whose labels a context keeps


def _ptr(t):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        if not t.is_cuda:
            raise PbrError("expected a device tensor")
        if not t.is_contiguous():
            raise PbrError("expected a contiguous tensor")
        return C.c_void_p(t.data_ptr())
    return C.c_void_p(int(t))


def _some(name, t):
    """t, a device buffer the textured and culled raster forwards cannot do without: in the descriptor a null one selects another raster"""
    if t is None or not _ptr(t).value:
        raise PbrError(f"pbr_gbuffer_raster: {name} null")
    return t


def _bc6h_faces(who, faces, size, mip_levels):
    """the six face chains of a BC6H cube (device tensors of structs.bc6h_chain_bytes each, or device addresses) as a pointer array;
    a description the library refuses is left to the library"""
    faces = list(faces)
    if len(faces) != 6:
        raise PbrError(f"{who}: six faces, got {len(faces)}")
    nbytes = bc6h_chain_bytes(size, mip_levels)
    for f in faces:
        if isinstance(f, torch.Tensor) and nbytes and f.numel() * f.element_size() != nbytes:
            raise PbrError(f"{who}: a face of {f.numel() * f.element_size()} bytes, {size}^2 x {mip_levels} levels takes {nbytes}")
    return (C.c_void_p * 6)(*[_ptr(f) for f in faces])


def _gbuffer(gb, pitch):
    """pbr_gbuffer of a dict with the device tensors A, B, C, depth, stencil"""
    return GBuffer(gb["A"].data_ptr(), gb["B"].data_ptr(), gb["C"].data_ptr(), gb["depth"].data_ptr(), gb["stencil"].data_ptr(), pitch)


class PbrContext:
    """One context per device per host thread (pbr_ctx is not thread-safe)."""

    def __init__(self, device=0, use_torch_stream=True):
        self.lib = _lib.load()
        self.device = int(device)
        h = C.c_void_p()
        st = self.lib.pbr_ctx_create(self.device, C.byref(h))
        if st != 0:
            raise PbrError(f"pbr_ctx_create({device}) failed: status {st}")
        self.h = h
        self.torch_device = torch.device("cuda", self.device)
        if use_torch_stream:
            self.bind_torch_stream()

    def bind_torch_stream(self):
        """Enqueue on torch's current stream so torch allocations/events order with our kernels."""
        s = torch.cuda.current_stream(self.torch_device)
        self._check(self.lib.pbr_ctx_set_stream(self.h, C.c_void_p(s.cuda_stream)))

    def close(self):
        if getattr(self, "h", None):
            self.lib.pbr_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != 0:
            msg = self.lib.pbr_last_error(self.h)
            raise PbrError(f"status {st}: {msg.decode() if msg else '?'}")

    def launch_log(self, last=LAUNCH_LOG):
        """pbr_launch_log: (launches since the context was created, the labels of the last min(last, 64, that many), oldest first).
        Which kernel an entry point chose is read here, e.g. count before, call, labels of the count's increase."""
        out = (C.c_char_p * LAUNCH_LOG)()
        total = int(self.lib.pbr_launch_log(self.h, C.cast(out, C.c_void_p), min(int(last), LAUNCH_LOG)))
        return total, [out[i].decode() for i in range(min(total, int(last), LAUNCH_LOG))]

    def launches_of(self, call):
        """run call() and return the labels of the kernels it launched (at most the last 64)"""
        before = self.launch_log(0)[0]
        call()
        total = self.launch_log(0)[0]
        return self.launch_log(total - before)[1]

    def side_begin(self):
        """Calls until side_end() enqueue on the context's high-priority side stream (after all earlier work)."""
        self._check(self.lib.pbr_ctx_side_begin(self.h))

    def side_end(self):
        self._check(self.lib.pbr_ctx_side_end(self.h))

    def side_join(self):
        """The context's stream waits for the side stream."""
        self._check(self.lib.pbr_ctx_side_join(self.h))

    def sync(self):
        self._check(self.lib.pbr_sync(self.h))

    def use_own_stream(self):
        """Enqueue on the context's private stream (not torch's): the caller orders torch work with ctx.sync() / torch.cuda.synchronize()."""
        self._check(self.lib.pbr_ctx_use_own_stream(self.h))

    def set_bloom_shader_order(self, on):
        """pbr_ctx_set_bloom_shader_order: the large 2x-up bloom levels in the shader's operation order (bit-exact at any size) instead
        of the polyphase form (<= 1 fp16 ULP per stage)"""
        self._check(self.lib.pbr_ctx_set_bloom_shader_order(self.h, 1 if on else 0))

    def partition_cus(self, side_cus, total_cus=None, layout="low", allow_uneven=False):
        """pbr_ctx_set_cu_masks with `side_cus` compute units, spread evenly over the device, for the side stream and the rest for the
        context's private stream (0: no partition, every CU for both).  The context must be on its private stream (use_own_stream).
        Masked streams synchronise with the legacy null stream (hipExtStreamCreateWithCUMask takes no flags): default-stream torch work
        (.zero_(), event records) or a hipMemset inside a partitioned frame makes the two partitions take turns.
        layout="low" needs side_cus to be a multiple of 32 (the same number of CUs from every XCD): anything else runs at the pace of
        the poorest XCD and is refused — the uneven layouts exist as "strided" / "per_xcd", for the measurement of exactly that;
        allow_uneven=True (tools/cu_partition.py, which measures that effect with layout "low" too) lifts the refusal."""
        if not hasattr(self.lib, "pbr_ctx_set_cu_masks"):
            raise PbrError("partition_cus: pbr_ctx_set_cu_masks is an entry point of the knobs build only (PBR_HIP_LIB=.../libpbr_hip_knobs.so): "
                           "the CU partition is a measurement aid, not part of the product library (round 6)")
        if side_cus and layout == "low" and int(side_cus) % 32 and not allow_uneven:
            raise PbrError(f"partition_cus: layout 'low' takes a multiple of 32 compute units (got {side_cus}): an uneven share per XCD runs at the poorest XCD's pace")
        if not side_cus:
            self._check(self.lib.pbr_ctx_set_cu_masks(self.h, None, None, 0))
            return
        n = int(total_cus or torch.cuda.get_device_properties(self.torch_device).multi_processor_count)
        words = (n + 31) // 32
        side = np.zeros(words, np.uint32)
        main = np.zeros(words, np.uint32)
        # On MI355X the bits of a CU mask run XCD by XCD in groups of four (measured: tools/cu_partition.py), and a kernel's workgroups
        # are dealt to the XCDs in equal shares whatever their CU counts — so both partitions must hold the SAME number of CUs of every
        # XCD, or the XCD with the fewest sets the pace: the side stream gets the low side_cus bits, side_cus a multiple of 32
        # (layout="strided": every (n / side_cus)-th bit instead, for the measurement of exactly that effect).
        if layout == "low":          # the low side_cus bits: even per XCD only for multiples of 32
            picked = set(range(side_cus))
        elif layout == "per_xcd":    # side_cus / 8 CUs of EVERY XCD (bit = 32 * (j // 4) + 4 * xcd + j % 4 for the j-th CU of an XCD)
            k = side_cus // 8
            picked = set(32 * (j // 4) + 4 * x + (j % 4) for x in range(8) for j in range(k))
        else:                        # "strided": every (n / side_cus)-th bit — uneven per XCD, for the measurement of exactly that effect
            picked = set(int(round(i * n / side_cus)) % n for i in range(side_cus))
        for cu in range(n):
            (side if cu in picked else main)[cu // 32] |= np.uint32(1 << (cu % 32))
        self._check(self.lib.pbr_ctx_set_cu_masks(self.h, main.ctypes.data, side.ctypes.data, words))

    # ---- allocation helpers (torch = device memory plumbing) ---------------------------------
    def empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.torch_device)

    def zeros(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype, device=self.torch_device)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        if arr.dtype in (LIGHT_DTYPE, CLUSTER_DTYPE, VERTEX_DTYPE, DRAW_DTYPE, DRAW_MAPS_DTYPE, AABB_DTYPE):
            arr = arr.view(np.uint8)
        if arr.dtype == np.uint32:
            return torch.from_numpy(arr.view(np.int32)).to(self.torch_device)
        if arr.dtype == np.uint16:
            return torch.from_numpy(arr.view(np.int16)).to(self.torch_device)
        return torch.from_numpy(arr).to(self.torch_device)

    # ---- one-shot IBL --------------------------------------------------------------------------
    def brdf_lut(self, res, out=None):
        out = out if out is not None else self.empty((res, res, 2), torch.float16)
        self._check(self.lib.pbr_brdf_lut(self.h, res, _ptr(out)))
        return out

    def cube_gen_mips(self, cube, size, mips):
        self._check(self.lib.pbr_cube_gen_mips(self.h, _ptr(cube), size, mips))
        return cube

    def prefilter_env(self, sky, sky_size, sky_mips, size=512, mips=ENV_MIPS, out=None):
        out = out if out is not None else self.empty((cube_texels(size, mips), 4), torch.float16)
        c = CubeF32(sky.data_ptr(), sky_size, sky_mips)
        self._check(self.lib.pbr_prefilter_env(self.h, C.byref(c), size, mips, _ptr(out)))
        return out

    def prefilter_env_dispatches(self, sky, sky_size, sky_mips, size=512, mips=ENV_MIPS, out=None):
        """The chain as PreFilterEnvMapPass::Execute builds it: ONE pbr_prefilter_env_mip per mip (the shader's sequential
        sum, roughness = mip / (mips - 1), DeferredPipeline.cpp:99) — what the C++ pass graph dispatches."""
        from .structs import cube_mip_offset
        out = out if out is not None else self.empty((cube_texels(size, mips), 4), torch.float16)
        c = CubeF32(sky.data_ptr(), sky_size, sky_mips)
        for m in range(mips):
            dst = out.data_ptr() + 8 * cube_mip_offset(size, m)
            self._check(self.lib.pbr_prefilter_env_mip(self.h, C.byref(c), size, m, float(m) / float(max(mips - 1, 1)), C.c_void_p(dst)))
        return out

    def env_pad(self, env, size, mips=ENV_MIPS, out=None):
        """Padded copy of a prefiltered env chain — the layout deferred_shade samples (one-shot)."""
        out = out if out is not None else self.empty((env_padded_texels(size, mips), 4), torch.float16)
        self._check(self.lib.pbr_env_pad(self.h, _ptr(env), size, mips, _ptr(out)))
        return out

    def bc6h_decode_cube(self, faces, size, mip_levels, out=None):
        """pbr_bc6h_decode_cube: the six BC6H_UF16 face chains of a sky asset -> the fp32 RGBA cube chain every consumer takes
        (float32 [cube_texels(size, mip_levels), 4], alpha 1).  faces: six device tensors (uint8, structs.bc6h_chain_bytes each) or
        six device addresses (e.g. into one uploaded file, at host.parse_cubemap_file's offsets), in the order px, nx, py, ny, pz, nz."""
        ptrs = _bc6h_faces("bc6h_decode_cube", faces, size, mip_levels)
        if out is None:
            if not bc6h_chain_bytes(size, mip_levels):
                raise PbrError(f"bad BC6H cube description: {size}^2, {mip_levels} levels")
            out = self.empty((cube_texels(size, mip_levels), 4), torch.float32)
        self._check(self.lib.pbr_bc6h_decode_cube(self.h, C.byref(ptrs), int(size), int(mip_levels), _ptr(out)))
        return out

    def bc6h_encode_cube(self, cube, size, mip_levels, out=None, two_region=False):
        """pbr_bc6h_encode_cube_ex, the inverse of bc6h_decode_cube: the fp32 RGBA cube chain (device float32 [cube_texels(size,
        mip_levels), 4]; alpha ignored) -> six BC6H_UF16 face chains (device uint8, structs.bc6h_chain_bytes each), in the order px, nx,
        py, ny, pz, nz.  out: six device tensors of that size or six device addresses to write to instead.  two_region: the ten
        two-region modes are candidates as well (PBR_BC6H_ENCODE_TWO_REGION); without it the four one-region modes, as before."""
        nbytes = bc6h_chain_bytes(size, mip_levels)
        if isinstance(cube, torch.Tensor) and nbytes and cube.numel() * cube.element_size() != 16 * cube_texels(size, mip_levels):
            raise PbrError(f"bc6h_encode_cube: a cube of {cube.numel() * cube.element_size()} bytes, {size}^2 x {mip_levels} levels takes "
                           f"{16 * cube_texels(size, mip_levels)}")
        if out is None:
            if not nbytes:
                raise PbrError(f"bad BC6H cube description: {size}^2, {mip_levels} levels")
            out = [self.empty((nbytes,), torch.uint8) for _ in range(6)]
        out = list(out)
        ptrs = _bc6h_faces("bc6h_encode_cube", out, size, mip_levels)
        self._check(self.lib.pbr_bc6h_encode_cube_ex(self.h, _ptr(cube), int(size), int(mip_levels), C.byref(ptrs),
                                                     BC6H_ENCODE_TWO_REGION if two_region else 0))
        return out

    def import_sky(self, level0, mip_levels=None, two_region=False):
        """The reference's ImportCubeMap from decoded faces on: level 0 (host float32 [6, size, size, 4] or the flat equivalent) is
        uploaded, its box mips made (cube_gen_mips), the SH pack projected from the fp32 level 0 — before compression, where the
        reference computes it — and the chain compressed (bc6h_encode_cube).  Returns (faces, sh_pack): six device uint8 chains and
        the 28 floats on the device; host.write_cubemap_file of their host copies is the sky's file.  two_region: bc6h_encode_cube's."""
        lv0 = np.ascontiguousarray(level0, dtype=np.float32).reshape(-1, 4)
        size = int(round((len(lv0) // 6) ** 0.5))
        if 6 * size * size != len(lv0):
            raise PbrError(f"import_sky: level 0 of {len(lv0)} texels is not six square faces")
        mips = size.bit_length() if mip_levels is None else int(mip_levels)
        if not bc6h_chain_bytes(size, mips):
            raise PbrError(f"bad BC6H cube description: {size}^2, {mips} levels")
        cube = self.empty((cube_texels(size, mips), 4), torch.float32)
        cube[:len(lv0)].copy_(torch.from_numpy(lv0))
        self.cube_gen_mips(cube, size, mips)
        sh = self.sh9_project(cube, size, mips)
        return self.bc6h_encode_cube(cube, size, mips, two_region=two_region), sh

    def equirect_to_cube(self, pano, pw, ph, size, samples=1, rgbe=False, out=None):
        """pbr_equirect_to_cube: an equirectangular panorama (device; float32 [ph, pw, 4], or with rgbe uint8 [ph, pw, 4] Radiance
        texels, decoded where they are fetched) -> level 0 of a sky cube, device float32 [6 size^2, 4], faces px, nx, py, ny, pz, nz,
        alpha 1: bilinear taps (longitude wraps, latitude clamps), samples^2 sub-samples per texel, samples one of 1, 2, 4, 8.  out: a
        device float32 tensor of at least 6 size^2 texels (a cube chain, say) whose level 0 is written instead."""
        if isinstance(pano, torch.Tensor) and pano.numel() * pano.element_size() != int(pw) * int(ph) * (4 if rgbe else 16):
            raise PbrError(f"equirect_to_cube: a panorama of {pano.numel() * pano.element_size()} bytes, {pw} x {ph} "
                           f"{'RGBE' if rgbe else 'fp32'} texels take {int(pw) * int(ph) * (4 if rgbe else 16)}")
        if out is None:
            if not 1 <= int(size) <= BC6H_MAX_SIZE:
                raise PbrError(f"equirect_to_cube: size {size} is not 1 .. {BC6H_MAX_SIZE}")
            out = self.empty((6 * int(size) * int(size), 4), torch.float32)
        elif isinstance(out, torch.Tensor) and out.numel() * out.element_size() < 96 * int(size) * int(size):
            raise PbrError(f"equirect_to_cube: out holds {out.numel() * out.element_size()} bytes, level 0 of size {size} takes {96 * int(size) * int(size)}")
        self._check(self.lib.pbr_equirect_to_cube(self.h, _ptr(pano), int(pw), int(ph), _ptr(out), int(size), int(samples),
                                                  EQUIRECT_SRC_RGBE if rgbe else 0))
        return out

    def import_sky_equirect(self, pano_host, size=None, samples=None, mip_levels=None, two_region=False):
        """import_sky with equirect_to_cube in front: one equirectangular panorama (host float32 [ph, pw, 4], or uint8 [ph, pw, 4]
        Radiance RGBE texels, which are uploaded as they are and sampled in place) is resampled into level 0, then the box mips, the SH
        pack of the fp32 level 0 and the BC6H_UF16 chains as import_sky makes them.  size / samples None: the default rules
        (structs.equirect_default_size / equirect_default_samples).  Returns (faces, sh_pack) exactly as import_sky does."""
        pano = np.ascontiguousarray(pano_host)
        if pano.ndim != 3 or pano.shape[2] != 4 or pano.dtype not in (np.dtype(np.float32), np.dtype(np.uint8)):
            raise PbrError(f"import_sky_equirect: a panorama is float32 or uint8 [ph, pw, 4], got {pano.dtype} {pano.shape}")
        ph, pw = pano.shape[:2]
        size = equirect_default_size(pw) if size is None else int(size)
        samples = equirect_default_samples(pw, size) if samples is None else int(samples)
        mips = size.bit_length() if mip_levels is None else int(mip_levels)
        if not bc6h_chain_bytes(size, mips):
            raise PbrError(f"bad BC6H cube description: {size}^2, {mips} levels")
        cube = self.empty((cube_texels(size, mips), 4), torch.float32)
        dev = self.upload(pano)
        self.equirect_to_cube(dev, pw, ph, size, samples, rgbe=pano.dtype == np.uint8, out=cube)
        self.cube_gen_mips(cube, size, mips)
        sh = self.sh9_project(cube, size, mips)
        return self.bc6h_encode_cube(cube, size, mips, two_region=two_region), sh

    def sh9_project(self, sky, sky_size, sky_mips=1, out=None):
        out = out if out is not None else self.empty((28,), torch.float32)
        c = CubeF32(sky.data_ptr(), sky_size, sky_mips)
        self._check(self.lib.pbr_sh9_project(self.h, C.byref(c), _ptr(out)))
        return out

    # ---- per-frame -------------------------------------------------------------------------------
    def alloc_clusters(self):
        return self.zeros((NUM_CLUSTERS * CLUSTER_DTYPE.itemsize,), torch.uint8)

    def cluster_build(self, g: Global, clusters):
        self._check(self.lib.pbr_cluster_build(self.h, C.byref(g), _ptr(clusters)))

    def cluster_cull(self, g: Global, lights, n, clusters):
        self._check(self.lib.pbr_cluster_cull(self.h, C.byref(g), _ptr(lights), int(n), _ptr(clusters)))

    def clustered(self, g: Global, lights, n, clusters):
        """cluster_build + cluster_cull in one launch (ClusteredPass::Execute)."""
        self._check(self.lib.pbr_clustered(self.h, C.byref(g), _ptr(lights), int(n), _ptr(clusters)))

    def _shade(self, g, tile, gb, pitch, lut, lut_fold, lut_res, env, env_size, env_mips, clusters, lights, num_lights, hdr, hdr_pitch,
               rects=None, tables=None, hdr_f32=None):
        """ONE pbr_deferred_shade (hdr_f32: pbr_deferred_shade_f32) call of a ShadeDesc; the G-buffer struct and the rectangle array live
        until it returns"""
        s = _gbuffer(gb, pitch)
        arr = self._rects(rects) if rects is not None else None
        d = ShadeDesc(C.addressof(g), C.addressof(tile), C.addressof(s), _ptr(lut), _ptr(lut_fold), _ptr(env), _ptr(clusters), _ptr(lights), _ptr(hdr),
                      C.addressof(arr) if arr is not None else None, C.addressof(tables) if tables is not None else None,
                      lut_res, env_size, env_mips, int(num_lights), hdr_pitch, len(arr) if arr is not None else 0)
        if hdr_f32 is None:
            self._check(self.lib.pbr_deferred_shade(self.h, C.byref(d)))
        else:
            self._check(self.lib.pbr_deferred_shade_f32(self.h, C.byref(d), _ptr(hdr_f32)))

    @staticmethod
    def _rects(rects):
        arr = ((C.c_uint32 * 4) * len(rects))()
        for i, r in enumerate(rects):
            arr[i] = (C.c_uint32 * 4)(*[int(v) for v in r])
        return arr

    def deferred_shade(self, g: Global, tile: Tile, gb, pitch, lut, lut_res, env, env_size, env_mips,
                       clusters, lights, num_lights, hdr, hdr_pitch):
        """gb: dict with device tensors A,B,C,depth,stencil; env: the PADDED chain from env_pad()."""
        self._shade(g, tile, gb, pitch, lut, None, lut_res, env, env_size, env_mips, clusters, lights, num_lights, hdr, hdr_pitch)

    def deferred_shade_rects(self, g: Global, tile: Tile, gb, pitch, lut, lut_res, env, env_size, env_mips,
                             clusters, lights, num_lights, hdr, hdr_pitch, rects):
        """deferred_shade on up to 5 rectangles (tile-local x, y, w, h) of the tile in one launch."""
        self._shade(g, tile, gb, pitch, lut, None, lut_res, env, env_size, env_mips, clusters, lights, num_lights, hdr, hdr_pitch, rects)

    def lut_fold_x(self, lut, lut_res, out=None):
        """The x-folded LUT the *_folded shades read (one-shot per LUT): float32 [lut_res, 256, 2], entry [y, rb] = the x-lerps of
        LUT row y's two channels at roughness byte rb, the very fp32 values deferred_shade computes per pixel."""
        out = out if out is not None else self.empty((int(lut_res), 256, 2), torch.float32)
        self._check(self.lib.pbr_lut_fold_x(self.h, _ptr(lut), int(lut_res), _ptr(out)))
        return out

    def deferred_shade_folded(self, g: Global, tile: Tile, gb, pitch, lut_fold, lut_res, env, env_size, env_mips,
                              clusters, lights, num_lights, hdr, hdr_pitch, rects=None):
        """deferred_shade (rects: deferred_shade_rects) with the LUT read from lut_fold_x()'s table: the same bits, fewer instructions."""
        self._shade(g, tile, gb, pitch, None, lut_fold, lut_res, env, env_size, env_mips, clusters, lights, num_lights, hdr, hdr_pitch, rects)

    def alloc_shade_tables(self, w, h):
        """The shade tables of a w x h tile: (device tensor, ShadeTables descriptor) with neither half built.  The tensor is the memory the
        descriptor points into: keep both."""
        n = int(self.lib.pbr_shade_tables_bytes(int(w), int(h)))
        buf = self.zeros((n // 4,), torch.int32)
        return buf, ShadeTables(buf.data_ptr(), n, 0, 0, 0, Tile(0, 0, 0, 0, 0, 0))

    def clustered_tables(self, g: Global, lights, n, clusters, tables: ShadeTables):
        """clustered() that also writes the frame half of the shade tables (light planes, q_safe, staged cluster lists) in the same launch."""
        self._check(self.lib.pbr_clustered_tables(self.h, C.byref(g), _ptr(lights), int(n), _ptr(clusters), C.byref(tables)))

    def shade_geometry_tables(self, tile: Tile, tables: ShadeTables):
        """The geometry half of the shade tables (column and row terms of the tile): once per target."""
        self._check(self.lib.pbr_shade_geometry_tables(self.h, C.byref(tile), C.byref(tables)))

    def deferred_shade_tabled(self, g: Global, tile: Tile, gb, pitch, lut_fold, lut_res, env, env_size, env_mips,
                              clusters, lights, num_lights, hdr, hdr_pitch, tables: ShadeTables, rects=None):
        """deferred_shade_folded whose blocks read their prologue from the shade tables (both halves built for this tile and light count)."""
        self._shade(g, tile, gb, pitch, None, lut_fold, lut_res, env, env_size, env_mips, clusters, lights, num_lights, hdr, hdr_pitch, rects, tables)

    def deferred_shade_f32(self, g: Global, tile: Tile, gb, pitch, lut, lut_res, env, env_size, env_mips,
                           clusters, lights, num_lights, hdr_f32, hdr_pitch):
        """Parity probe: deferred_shade with a float32 [h, w, 4] output (the colour before the fp16 store)."""
        self._shade(g, tile, gb, pitch, lut, None, lut_res, env, env_size, env_mips, clusters, lights, num_lights, None, hdr_pitch, hdr_f32=hdr_f32)

    def rgbe_decode(self, rgbe, out):
        """rgbe: uint8 device tensor [..., 4] (Radiance texels); out: float32 [..., 4]."""
        self._check(self.lib.pbr_rgbe_decode(self.h, _ptr(rgbe), rgbe.numel() // 4, _ptr(out)))

    def skybox(self, g: Global, tile: Tile, sky, sky_size, sky_mips, stencil, pitch, hdr, hdr_pitch):
        """skybox.hlsl: sky colour into hdr where stencil == 0 (run before deferred_shade)."""
        c = CubeF32(sky.data_ptr(), sky_size, sky_mips)
        self._check(self.lib.pbr_skybox(self.h, C.byref(g), C.byref(tile), C.byref(c), _ptr(stencil), pitch,
                                        _ptr(hdr), hdr_pitch))

    def skybox_bc6h(self, g: Global, tile: Tile, faces, size, mip_levels, stencil, pitch, hdr, hdr_pitch):
        """pbr_skybox_bc6h: the sky pass on a cube that stays resident as BC6H_UF16 blocks, sampled in place — the bits skybox() writes
        from the cube bc6h_decode_cube makes of the same chains.  faces: six device tensors (uint8, structs.bc6h_chain_bytes each) or
        six device addresses (16-byte aligned), in the order px, nx, py, ny, pz, nz."""
        c = CubeBc6h(_bc6h_faces("skybox_bc6h", faces, size, mip_levels), int(size), int(mip_levels))
        self._check(self.lib.pbr_skybox_bc6h(self.h, C.byref(g), C.byref(tile), C.byref(c), _ptr(stencil), pitch,
                                             _ptr(hdr), hdr_pitch))

    def gbuffer_encode(self, m0, m1, m2, w, h, pitch, A, B, Cc):
        """gbuffer.hlsl::ps_main on per-pixel material planes (float4 each) -> RGBA8 G-buffer planes."""
        self._check(self.lib.pbr_gbuffer_encode(self.h, _ptr(m0), _ptr(m1), _ptr(m2), w, h, pitch,
                                                _ptr(A), _ptr(B), _ptr(Cc)))

    # ---- G-buffer rasterization ----------------------------------------------------------------
    def _raster_scratch(self, call, w, h, n_triangles, minimum, extra=None):
        """pbr_<call>_scratch_bytes (recommended) or, minimum, pbr_<call>_min_scratch_bytes for a w x h tile; with extra, a device
        tensor of that many bytes and `extra` more (uint8; 256-byte aligned like every torch allocation)"""
        nbytes = int(getattr(self.lib, f"pbr_{call}_{'min_' if minimum else ''}scratch_bytes")(int(w), int(h), int(n_triangles)))
        return nbytes if extra is None else self.empty((nbytes + int(extra),), torch.uint8)

    def raster_scratch_bytes(self, w, h, n_triangles, minimum=False):
        """pbr_gbuffer_raster_scratch_bytes (recommended) or, minimum=True, pbr_gbuffer_raster_min_scratch_bytes for a w x h tile"""
        return self._raster_scratch("gbuffer_raster", w, h, n_triangles, minimum)

    def alloc_raster_scratch(self, w, h, n_triangles, minimum=False, extra=0):
        """device scratch for gbuffer_raster"""
        return self._raster_scratch("gbuffer_raster", w, h, n_triangles, minimum, extra)

    def gbuffer_raster(self, g: Global, tile: Tile, vertices, n_vertices, indices, n_indices, draws, n_draws, max_triangles,
                       A, B, Cc, depth, stencil, pitch, scratch, scratch_bytes=None, *, maps=None, textures=None, bounds=None, stats=None):
        """pbr_gbuffer_raster, the one call that fills a RasterDesc: draws (device structs.DRAW_DTYPE records) of the vertex / index
        buffers (device VERTEX_DTYPE records, uint32 indices) -> the tile's five G-buffer planes.  max_triangles = sum of
        index_count // 3; scratch from alloc_raster_scratch.  maps, textures, bounds, stats: as gbuffer_raster_textured and
        gbuffer_raster_culled describe them; with maps the scratch is alloc_textured_raster_scratch's."""
        textures = list(textures or ())
        table = (Texture2D * len(textures))(*textures)
        nbytes = scratch.numel() * scratch.element_size() if scratch_bytes is None else int(scratch_bytes)
        d = RasterDesc(C.addressof(g), C.addressof(tile), _ptr(vertices), _ptr(indices), _ptr(draws), _ptr(A), _ptr(B), _ptr(Cc),
                       _ptr(depth), _ptr(stencil), _ptr(scratch), nbytes, _ptr(maps), C.addressof(table) if textures else None, _ptr(bounds),
                       _ptr(stats), int(n_vertices), int(n_indices), int(n_draws), int(max_triangles), int(pitch), len(textures))
        self._check(self.lib.pbr_gbuffer_raster(self.h, C.byref(d)))

    def depth_raster_scratch_bytes(self, w, h, n_triangles, minimum=False):
        """pbr_depth_raster_scratch_bytes (recommended) or, minimum=True, pbr_depth_raster_min_scratch_bytes for a w x h tile"""
        return self._raster_scratch("depth_raster", w, h, n_triangles, minimum)

    def alloc_depth_raster_scratch(self, w, h, n_triangles, minimum=False, extra=0):
        """device scratch for depth_raster: gbuffer_raster's without the 80-byte resolve record per triangle"""
        return self._raster_scratch("depth_raster", w, h, n_triangles, minimum, extra)

    def depth_raster(self, g: Global, tile: Tile, vertices, n_vertices, indices, n_indices, draws, n_draws, max_triangles, depth, pitch,
                     scratch, scratch_bytes=None, *, bounds=None, stats=None):
        """pbr_depth_raster: the depth plane of gbuffer_raster (without maps), bit for bit, and nothing else — a shadow map or a
        depth pre-pass at 4 bytes per texel.  The arguments are gbuffer_raster's without the other four planes; scratch from
        alloc_depth_raster_scratch; bounds and stats as gbuffer_raster_culled takes them."""
        nbytes = scratch.numel() * scratch.element_size() if scratch_bytes is None else int(scratch_bytes)
        d = DepthRasterDesc(C.addressof(g), C.addressof(tile), _ptr(vertices), _ptr(indices), _ptr(draws), _ptr(depth), _ptr(scratch), nbytes,
                            _ptr(bounds), _ptr(stats), int(n_vertices), int(n_indices), int(n_draws), int(max_triangles), int(pitch), 0)
        self._check(self.lib.pbr_depth_raster(self.h, C.byref(d)))

    def textured_raster_scratch_bytes(self, w, h, n_triangles, minimum=False):
        """pbr_gbuffer_raster_textured_scratch_bytes (recommended) or, minimum=True, its _min_scratch_bytes for a w x h tile"""
        return self._raster_scratch("gbuffer_raster_textured", w, h, n_triangles, minimum)

    def alloc_textured_raster_scratch(self, w, h, n_triangles, minimum=False, extra=0):
        """device scratch for gbuffer_raster_textured"""
        return self._raster_scratch("gbuffer_raster_textured", w, h, n_triangles, minimum, extra)

    def upload_texture(self, chain, width, height, mip_levels, fmt):
        """A texture's mip chain (host bytes in the reference's layout: scene.mip_chain / pack_chain) -> (device tensor,
        structs.Texture2D describing it).  Keep the tensor alive while the descriptor is in use.
        fmt | structs.TEX_BC1_BLOCKS: the chain is BC1 blocks (the payload of the reference's texture files), kept as they are for
        the rasterizer to sample in place; its byte count must be structs.texture2d_bytes of the description."""
        fmt = int(fmt)
        host = np.ascontiguousarray(chain).view(np.uint8).reshape(-1)
        if fmt & TEX_BC1_BLOCKS:
            want = texture2d_bytes(width, height, mip_levels, fmt)
            if want == 0:
                raise PbrError(f"bad BC1 texture description: {width} x {height}, {mip_levels} levels, format {fmt:#x}")
            if host.size != want:
                raise PbrError(f"BC1 chain of {host.size} bytes, {width} x {height} x {mip_levels} levels takes {want}")
        elif fmt not in TEX_FORMATS:
            raise PbrError(f"unknown texture format {fmt}")
        dev = self.upload(host)
        return dev, Texture2D(dev.data_ptr(), int(width), int(height), int(mip_levels), fmt)

    def bc1_decode(self, blocks, width, height, mip_levels, stored_format, out=None):
        """pbr_bc1_decode: a BC1 chain on the device (uint8 tensor, or the (tensor, Texture2D) pair of upload_texture) -> the
        decoded chain in stored_format as upload_texture returns it: (device tensor, structs.Texture2D)."""
        if isinstance(blocks, tuple):
            blocks = blocks[0]
        nbytes = texture2d_bytes(width, height, mip_levels, int(stored_format))
        if nbytes == 0 or int(stored_format) & TEX_BC1_BLOCKS:
            raise PbrError(f"bad texture description: {width} x {height}, {mip_levels} levels, stored format {stored_format}")
        if blocks.numel() * blocks.element_size() != texture2d_bytes(width, height, mip_levels, int(stored_format) | TEX_BC1_BLOCKS):
            raise PbrError("bc1_decode: the block tensor's size does not match the description")
        out = out if out is not None else self.empty((nbytes,), torch.uint8)
        self._check(self.lib.pbr_bc1_decode(self.h, _ptr(blocks), int(width), int(height), int(mip_levels), int(stored_format), _ptr(out)))
        return out, Texture2D(out.data_ptr(), int(width), int(height), int(mip_levels), int(stored_format))

    def texture2d_gen_mips(self, chain, width, height, mip_levels, fmt):
        """pbr_texture2d_gen_mips: levels 1 .. mip_levels - 1 of the uncompressed chain on the device (uint8 tensor of
        structs.texture2d_bytes, level 0 filled), in place, by scene.mip_chain's rule."""
        if isinstance(chain, tuple):
            chain = chain[0]
        nbytes = texture2d_bytes(width, height, mip_levels, int(fmt))
        if nbytes == 0 or int(fmt) & TEX_BC1_BLOCKS:
            raise PbrError(f"bad texture description: {width} x {height}, {mip_levels} levels, format {fmt}")
        if chain.numel() * chain.element_size() != nbytes:
            raise PbrError("texture2d_gen_mips: the chain tensor's size does not match the description")
        self._check(self.lib.pbr_texture2d_gen_mips(self.h, _ptr(chain), int(width), int(height), int(mip_levels), int(fmt)))

    def bc1_encode(self, texels, width, height, mip_levels, stored_format, out=None):
        """pbr_bc1_encode, the mirror image of bc1_decode: an uncompressed chain on the device (uint8 tensor, or the (tensor,
        Texture2D) pair of upload_texture) in stored_format -> its BC1 chain: (device tensor, structs.Texture2D with
        stored_format | TEX_BC1_BLOCKS), as upload_texture returns a BC1-resident texture."""
        if isinstance(texels, tuple):
            texels = texels[0]
        fmt = int(stored_format)
        nbytes = texture2d_bytes(width, height, mip_levels, fmt | TEX_BC1_BLOCKS)
        if nbytes == 0 or fmt & TEX_BC1_BLOCKS:
            raise PbrError(f"bad texture description: {width} x {height}, {mip_levels} levels, stored format {stored_format}")
        if texels.numel() * texels.element_size() != texture2d_bytes(width, height, mip_levels, fmt):
            raise PbrError("bc1_encode: the texel tensor's size does not match the description")
        out = out if out is not None else self.empty((nbytes,), torch.uint8)
        if out.numel() * out.element_size() != nbytes:
            raise PbrError("bc1_encode: the output tensor's size does not match the description")
        self._check(self.lib.pbr_bc1_encode(self.h, _ptr(texels), int(width), int(height), int(mip_levels), fmt, _ptr(out)))
        return out, Texture2D(out.data_ptr(), int(width), int(height), int(mip_levels), fmt | TEX_BC1_BLOCKS)

    def import_texture(self, level0, fmt, mip_levels=None, bc1=False):
        """The reference's ImportTexture from decoded pixels on: host level 0 (uint8 [h, w] for R8, [h, w, 4] for the 4-byte
        formats, in the stored byte order of fmt) -> upload into a chain-sized buffer, texture2d_gen_mips (all levels by default),
        and with bc1=True bc1_encode -> the (device tensor, structs.Texture2D) pair DeferredFrame.set_meshes(..., textures=) and
        gbuffer_raster_textured take."""
        fmt = int(fmt)
        if fmt not in TEX_FORMATS:
            raise PbrError(f"unknown texture format {fmt}")
        lv0 = np.ascontiguousarray(level0, dtype=np.uint8)
        want_dims = 2 if TEX_FORMATS[fmt][0] == 1 else 3
        if lv0.ndim != want_dims or (want_dims == 3 and lv0.shape[2] != 4):
            raise PbrError(f"import_texture: level 0 of format {fmt} is uint8 {'[h, w]' if want_dims == 2 else '[h, w, 4]'}, got {lv0.shape}")
        h, w = lv0.shape[:2]
        mips = min(w, h).bit_length() if mip_levels is None else int(mip_levels)
        nbytes = texture2d_bytes(w, h, mips, fmt)
        if nbytes == 0:
            raise PbrError(f"bad texture description: {w} x {h}, {mips} levels, format {fmt}")
        chain = self.empty((nbytes,), torch.uint8)
        chain[:lv0.size].copy_(torch.from_numpy(lv0.reshape(-1)))
        self.texture2d_gen_mips(chain, w, h, mips, fmt)
        if bc1:
            return self.bc1_encode(chain, w, h, mips, fmt)
        return chain, Texture2D(chain.data_ptr(), w, h, mips, fmt)

    def gbuffer_raster_textured(self, g: Global, tile: Tile, vertices, n_vertices, indices, n_indices, draws, n_draws, max_triangles,
                                A, B, Cc, depth, stencil, pitch, scratch, maps, textures, scratch_bytes=None):
        """pbr_gbuffer_raster with maps: gbuffer_raster plus maps (device DRAW_MAPS_DTYPE records, one per draw) and textures (a
        sequence of structs.Texture2D, from upload_texture; host side, at most RASTER_MAX_TEXTURES).  Scratch from
        alloc_textured_raster_scratch."""
        self.gbuffer_raster(g, tile, vertices, n_vertices, indices, n_indices, draws, n_draws, max_triangles, A, B, Cc, depth, stencil,
                            pitch, scratch, scratch_bytes, maps=_some("maps", maps), textures=textures)

    # ---- model culling ---------------------------------------------------------------------------
    def draw_bounds(self, vertices, n_vertices, indices, n_indices, draws, n_draws, out=None):
        """pbr_draw_bounds: the draws' local boxes (device structs.AABB_DTYPE records as a [n_draws, 6] float32 tensor: min, max)
        from the device buffers the raster takes; asynchronous.  The host twin is scene.MeshScene.bounds / scene.draw_bounds."""
        out = out if out is not None else self.empty((int(n_draws), 6), torch.float32)
        self._check(self.lib.pbr_draw_bounds(self.h, _ptr(vertices), int(n_vertices), _ptr(indices), int(n_indices), _ptr(draws),
                                             int(n_draws), _ptr(out)))
        return out

    def alloc_cull_stats(self):
        """device pbr_cull_stats (4 x uint32 as int32) for the culled calls; read it back with read_cull_stats"""
        return self.zeros((4,), torch.int32)

    def read_cull_stats(self, stats):
        """structs.CullStats of a device record the culled calls wrote (synchronises)"""
        v = stats.cpu().numpy().view(np.uint32)
        return CullStats(int(v[0]), int(v[1]), int(v[2]), int(v[3]))

    def gbuffer_raster_culled(self, g: Global, tile: Tile, vertices, n_vertices, indices, n_indices, draws, n_draws, max_triangles,
                              A, B, Cc, depth, stencil, pitch, scratch, bounds, stats=None, scratch_bytes=None):
        """pbr_gbuffer_raster with bounds: gbuffer_raster plus bounds (device AABB_DTYPE records, one per draw: draw_bounds) and stats
        (device, alloc_cull_stats; None: not recorded).  A draw whose world box lies outside the widened tile's frustum is not set
        up; the planes are bit-identical to gbuffer_raster's."""
        self.gbuffer_raster(g, tile, vertices, n_vertices, indices, n_indices, draws, n_draws, max_triangles, A, B, Cc, depth, stencil,
                            pitch, scratch, scratch_bytes, bounds=_some("bounds", bounds), stats=stats)

    def gbuffer_raster_textured_culled(self, g: Global, tile: Tile, vertices, n_vertices, indices, n_indices, draws, n_draws,
                                       max_triangles, A, B, Cc, depth, stencil, pitch, scratch, maps, textures, bounds, stats=None,
                                       scratch_bytes=None):
        """pbr_gbuffer_raster with maps and bounds: gbuffer_raster_textured plus bounds and stats as gbuffer_raster_culled takes them"""
        self.gbuffer_raster(g, tile, vertices, n_vertices, indices, n_indices, draws, n_draws, max_triangles, A, B, Cc, depth, stencil,
                            pitch, scratch, scratch_bytes, maps=_some("maps", maps), textures=textures, bounds=_some("bounds", bounds),
                            stats=stats)

    def _bloom_prefilter(self, hdr, w, h, pitch, out, threshold, knee, out_pitch=0, out_x=0, out_y=0, rects=None):
        """ONE pbr_bloom_prefilter call of a BloomPrefilterDesc; the rectangle array lives until it returns"""
        arr = self._rects(rects) if rects is not None else None
        d = BloomPrefilterDesc(_ptr(hdr), _ptr(out), C.addressof(arr) if arr is not None else None, int(w), int(h), int(pitch),
                               int(out_pitch), int(out_x), int(out_y), len(arr) if arr is not None else 0, float(threshold), float(knee))
        self._check(self.lib.pbr_bloom_prefilter(self.h, C.byref(d)))

    def bloom_prefilter(self, hdr, w, h, pitch, out, threshold=BLOOM_THRESHOLD, knee=BLOOM_KNEE):
        self._bloom_prefilter(hdr, w, h, pitch, out, threshold, knee)

    def blur_h(self, src, iw, ih, out, ow, oh):
        self._check(self.lib.pbr_blur_h(self.h, _ptr(src), iw, ih, _ptr(out), ow, oh))

    def blur_v(self, src, iw, ih, out, ow, oh):
        self._check(self.lib.pbr_blur_v(self.h, _ptr(src), iw, ih, _ptr(out), ow, oh))

    def bloom_up_level(self, upper, lower, lw, lh, out, ow, oh):
        """out = V(H(upper) + H(lower at out's size)) — one fused upsample level (upper may be None)"""
        self._check(self.lib.pbr_bloom_up_level(self.h, _ptr(upper) if upper is not None else None, _ptr(lower), lw, lh, _ptr(out), ow, oh))

    def bloom_upsample_add(self, upper, uw, uh, lower, lw, lh, out):
        self._check(self.lib.pbr_bloom_upsample_add(self.h, _ptr(upper), uw, uh, _ptr(lower), lw, lh, _ptr(out)))

    def bloom_merge(self, hdr, pitch, src, w, h):
        self._check(self.lib.pbr_bloom_merge(self.h, _ptr(hdr), pitch, _ptr(src), w, h))

    def alloc_bloom_chain(self, w, h):
        return self.zeros((bloom_chain_texels(w, h), 4), torch.float16)

    def _bloom(self, hdr, w, h, hdr_pitch, chain_a, chain_b, threshold=0.0, knee=0.0, hdr_rect=None, merge_rect=None, hist_rect=None, hist=None,
               min_log=0.0, inv_range=0.0):
        """ONE pbr_bloom call of a BloomDesc; the rectangle arrays live until it returns"""
        rects = [self._rects([r]) if r is not None else None for r in (hdr_rect, merge_rect, hist_rect)]
        d = BloomDesc(_ptr(hdr), _ptr(chain_a), _ptr(chain_b), _ptr(hist), *[C.addressof(r) if r is not None else None for r in rects],
                      int(w), int(h), int(hdr_pitch), float(threshold), float(knee), float(min_log), float(inv_range))
        self._check(self.lib.pbr_bloom(self.h, C.byref(d)))

    def bloom(self, hdr, w, h, pitch, chain_a, chain_b, threshold=BLOOM_THRESHOLD, knee=BLOOM_KNEE):
        self._bloom(hdr, w, h, pitch, chain_a, chain_b, threshold, knee)

    def bloom_histogram(self, hdr, w, h, pitch, chain_a, chain_b, rect, hist, threshold=BLOOM_THRESHOLD, knee=BLOOM_KNEE,
                        min_log=MIN_LOG_LUMINANCE, inv_range=INV_LOG_LUMINANCE_RANGE):
        """bloom + luminance histogram of rect=(x,y,w,h) in one pass (adds into hist)."""
        self._bloom(hdr, w, h, pitch, chain_a, chain_b, threshold, knee, hist_rect=rect, hist=hist, min_log=min_log, inv_range=inv_range)

    def bloom_prefilter_rect(self, hdr, w, h, pitch, out, out_pitch, out_x, out_y, rect, threshold=BLOOM_THRESHOLD, knee=BLOOM_KNEE):
        """bloom_prefilter on the half-res outputs rect=(x,y,w,h) of the image, stored at (out_x + x, out_y + y) of `out`."""
        self._bloom_prefilter(hdr, w, h, pitch, out, threshold, knee, out_pitch, out_x, out_y, [rect])

    def bloom_prefilter_rects(self, hdr, w, h, pitch, out, out_pitch, out_x, out_y, rects, threshold=BLOOM_THRESHOLD, knee=BLOOM_KNEE):
        self._bloom_prefilter(hdr, w, h, pitch, out, threshold, knee, out_pitch, out_x, out_y, rects)

    def bloom_tiled(self, hdr, hdr_pitch, hdr_rect, ew, eh, chain_a, chain_b, merge_rect, hist=None,
                    min_log=MIN_LOG_LUMINANCE, inv_range=INV_LOG_LUMINANCE_RANGE):
        """Bloom levels 1..4 on the extended tile (level 1 of chain_a already complete) + merge/histogram of merge_rect."""
        self._bloom(hdr, ew, eh, hdr_pitch, chain_a, chain_b, hdr_rect=hdr_rect, merge_rect=merge_rect, hist=hist, min_log=min_log, inv_range=inv_range)

    def lum_histogram(self, hdr, w, h, pitch, hist, min_log=MIN_LOG_LUMINANCE, inv_range=INV_LOG_LUMINANCE_RANGE):
        self._check(self.lib.pbr_lum_histogram(self.h, _ptr(hdr), w, h, pitch, min_log, inv_range, _ptr(hist)))

    def lum_average(self, hist, pixel_count, dt, avg, min_log=MIN_LOG_LUMINANCE, log_range=LOG_LUMINANCE_RANGE):
        self._check(self.lib.pbr_lum_average(self.h, _ptr(hist), pixel_count, min_log, log_range, dt, _ptr(avg)))

    def tonemap(self, hdr, w, h, pitch, avg, out, out_pitch):
        self._check(self.lib.pbr_tonemap(self.h, _ptr(hdr), w, h, pitch, _ptr(avg), _ptr(out), out_pitch))

    def average_tonemap(self, hist, pixel_count, dt, avg_in, avg_out, hist_clear, hdr, w, h, pitch, out, out_pitch,
                        min_log=MIN_LOG_LUMINANCE, log_range=LOG_LUMINANCE_RANGE):
        """pbr_lum_average + pbr_tonemap as one launch: avg_out != avg_in, hist_clear != hist (see pbr_hip.h)"""
        self._check(self.lib.pbr_average_tonemap(self.h, _ptr(hist), pixel_count, min_log, log_range, dt, _ptr(avg_in), _ptr(avg_out),
                                                 _ptr(hist_clear) if hist_clear is not None else None, _ptr(hdr), w, h, pitch, _ptr(out), out_pitch))

    # ---- multi-view calls: `views` is a ctypes array of View (structs.View), n <= MAX_VIEWS equal-sized whole frames
    def clustered_views(self, views, n):
        self._check(self.lib.pbr_clustered_views(self.h, views, n))

    def deferred_shade_views(self, views, n, w, h, lut, lut_res, env, env_size, env_mips):
        """env: the PADDED chain from env_pad(); SkyBoxSH must be the same in every view"""
        self._check(self.lib.pbr_deferred_shade_views(self.h, views, n, w, h, _ptr(lut), lut_res, _ptr(env), env_size, env_mips))

    def bloom_histogram_views(self, views, n, w, h, threshold=BLOOM_THRESHOLD, knee=BLOOM_KNEE,
                              min_log=MIN_LOG_LUMINANCE, inv_range=INV_LOG_LUMINANCE_RANGE):
        self._check(self.lib.pbr_bloom_histogram_views(self.h, views, n, w, h, threshold, knee, min_log, inv_range))

    def lum_average_views(self, views, n, pixel_count, min_log=MIN_LOG_LUMINANCE, log_range=LOG_LUMINANCE_RANGE):
        self._check(self.lib.pbr_lum_average_views(self.h, views, n, pixel_count, min_log, log_range))

    def tonemap_views(self, views, n, w, h):
        self._check(self.lib.pbr_tonemap_views(self.h, views, n, w, h))

    def skybox_views(self, views, n, w, h, sky, sky_size, sky_mips):
        """pbr_skybox_views: skybox() of every view (g, gb.stencil, hdr) in one launch"""
        c = CubeF32(sky.data_ptr(), sky_size, sky_mips)
        self._check(self.lib.pbr_skybox_views(self.h, views, int(n), int(w), int(h), C.byref(c)))

    def skybox_bc6h_views(self, views, n, w, h, faces, size, mip_levels):
        """pbr_skybox_bc6h_views: skybox_bc6h() of every view in one launch; faces as skybox_bc6h takes them"""
        c = CubeBc6h(_bc6h_faces("skybox_bc6h_views", faces, size, mip_levels), int(size), int(mip_levels))
        self._check(self.lib.pbr_skybox_bc6h_views(self.h, views, int(n), int(w), int(h), C.byref(c)))

    # ---- anti-aliasing: an integer edge filter on RGBA8 images (include/pbr_hip.h, "Anti-aliasing")
    def fxaa(self, src, w, h, src_pitch, dst, dst_pitch):
        """pbr_fxaa: src -> dst, two RGBA8 device images (tensors or addresses) of w x h pixels, pitches in pixels.  dst must not overlap
        src; what the library refuses (a null pointer, an empty image, a pitch below w, an overlap) raises PbrError"""
        self._check(self.lib.pbr_fxaa(self.h, _ptr(src), int(w), int(h), int(src_pitch), _ptr(dst), int(dst_pitch)))

    def fxaa_batch(self, images, w, h):
        """pbr_fxaa_batch: images = up to MAX_VIEWS (src, src_pitch, dst, dst_pitch) tuples of equal-sized images, filtered in ONE launch;
        every dst gets the bits of its own fxaa() call"""
        images = list(images)
        arr = (FxaaImage * max(len(images), 1))()
        for i, (src, src_pitch, dst, dst_pitch) in enumerate(images):
            arr[i] = FxaaImage(_ptr(src), int(src_pitch), _ptr(dst), int(dst_pitch))
        self._check(self.lib.pbr_fxaa_batch(self.h, arr, len(images), int(w), int(h)))

    # ---- sun light with a shadow map (include/pbr_hip.h, "Sun light with a shadow map")
    def sun_light(self, g: Global, tile: Tile, gb, pitch, sun: Sun, hdr, hdr_pitch, shadow_depth=None, map_w=0, map_h=0, map_pitch=None,
                  contrib_f32=None):
        """pbr_sun_light: the directional light `sun` (structs.Sun, make_sun) added to the fp16 target hdr where the G-buffer gb (dict of
        device tensors A, B, C, depth, stencil) holds geometry; shadow_depth: the depth plane of a gbuffer_raster call under sun_fit's
        light camera (None: no shadows).  contrib_f32 (float32 [h, hdr_pitch, 4], hdr None): the parity probe, the contribution alone."""
        s = _gbuffer(gb, pitch)
        d = SunDesc(C.addressof(g), C.addressof(tile), C.addressof(s), C.addressof(sun), _ptr(shadow_depth), _ptr(hdr), _ptr(contrib_f32),
                    int(map_w), int(map_h), int(map_w if map_pitch is None else map_pitch), int(hdr_pitch))
        self._check(self.lib.pbr_sun_light(self.h, C.byref(d)))

    def sun_fit(self, direction, box_min, box_max, map_w, map_h):
        """pbr_sun_fit (host only): see the module's sun_fit"""
        return sun_fit(direction, box_min, box_max, map_w, map_h)

    def membench_read(self, buf, sink, blocks):
        """One streaming-read pass over `buf` (measurement aid: the device's achievable HBM-read bandwidth)."""
        self._check(self.lib.pbr_membench_read(self.h, _ptr(buf), buf.numel() * buf.element_size(), _ptr(sink), blocks))

    def valubench(self, op, blocks, iters, stamps):
        """pbr_valubench: blocks x 4 waves issue iters x 8 instructions of class op (0 v_mul_f32, 1 v_fma_f32, 2 v_pk_fma_f32,
        3 v_rcp_f32); stamps: int64 [blocks * 4, 4] device tensor = {shader cycles start, end, 100 MHz ticks start, end} per wave"""
        # the kernel writes blocks * 4 * 4 uint64 through the raw pointer: a short or mistyped tensor would be a silent out-of-bounds write
        if not (isinstance(stamps, torch.Tensor) and stamps.is_cuda and stamps.dtype == torch.int64 and stamps.is_contiguous()
                and stamps.numel() >= int(blocks) * 16):
            raise PbrError(f"valubench: stamps must be a contiguous int64 device tensor of at least {int(blocks) * 16} elements")
        self._check(self.lib.pbr_valubench(self.h, int(op), int(blocks), int(iters), _ptr(stamps)))

    # ---- multi-GPU --------------------------------------------------------------------------------
    def comm_init(self, world, rank, unique_id: bytes):
        buf = C.create_string_buffer(unique_id, 128) if unique_id is not None else None
        self._check(self.lib.pbr_comm_init(self.h, world, rank, C.cast(buf, C.c_void_p) if buf else None))

    def allreduce_hist(self, hist):
        self._check(self.lib.pbr_allreduce_hist(self.h, _ptr(hist)))

    @staticmethod
    def halo_peers(plan):
        """plan: [(rank, send_rect, recv_rect)] with rect = (x, y, w, h) in plane texels or None -> pbr_halo_peer array."""
        arr = (HaloPeer * max(len(plan), 1))()
        for i, (rank, send, recv) in enumerate(plan):
            arr[i].rank = int(rank)
            arr[i].send = (C.c_uint32 * 4)(*(send or (0, 0, 0, 0)))
            arr[i].recv = (C.c_uint32 * 4)(*(recv or (0, 0, 0, 0)))
        return arr, len(plan)

    def halo_staging_bytes(self, peers, n):
        return int(self.lib.pbr_halo_staging_bytes(peers, n))

    def halo_exchange(self, plane, pitch, rows, peers, n, staging):
        """RCCL send/recv of the plan's rectangles on the ctx communicator (pbr_comm_init first)."""
        self._check(self.lib.pbr_halo_exchange(self.h, _ptr(plane), pitch, rows, peers, n, _ptr(staging), staging.numel() * staging.element_size()))

    def halo_pack(self, plane, pitch, rows, peers, n, staging, unpack=False):
        self._check(self.lib.pbr_halo_pack(self.h, _ptr(plane), pitch, rows, peers, n, _ptr(staging),
                                           staging.numel() * staging.element_size(), 1 if unpack else 0))


def comm_unique_id() -> bytes:
    lib = _lib.load()
    buf = C.create_string_buffer(128)
    st = lib.pbr_comm_unique_id(C.cast(buf, C.c_void_p))
    if st != 0:
        raise PbrError(f"pbr_comm_unique_id failed: status {st}")
    return buf.raw


def sun_fit(direction, box_min, box_max, map_w, map_h):
    """pbr_sun_fit: (light Global, LightViewProj as 16 floats) of the orthographic light camera that looks along -direction and holds
    the world box [box_min, box_max] with one map texel of margin in x / y and 1 % in depth.  Host only: no context, no GPU."""
    lib = _lib.load()
    g, m = Global(), (C.c_float * 16)()
    box = Aabb((C.c_float * 3)(*[float(v) for v in box_min]), (C.c_float * 3)(*[float(v) for v in box_max]))
    st = lib.pbr_sun_fit(C.byref((C.c_float * 3)(*[float(v) for v in direction])), C.byref(box), int(map_w), int(map_h), C.byref(g), C.byref(m))
    if st != 0:
        raise PbrError(f"pbr_sun_fit refused (status {st}): direction {tuple(direction)}, box {tuple(box_min)} .. {tuple(box_max)}, map {map_w} x {map_h}")
    return g, [float(v) for v in m]


def make_sun(direction, luminance, light_view_proj=None, bias=(0.0, 0.0), pcf=3):
    """structs.Sun: direction normalised in double and rounded to float32, luminance a scalar or three channels, light_view_proj 16
    floats (None: the identity, for a light without a map)."""
    d = np.asarray(direction, dtype=np.float64).reshape(3)
    d = d / np.sqrt(float((d * d).sum()))
    lum = np.broadcast_to(np.asarray(luminance, dtype=np.float32), (3,))
    m = np.eye(4, dtype=np.float32).reshape(16) if light_view_proj is None else np.asarray(light_view_proj, dtype=np.float32).reshape(16)
    return Sun((C.c_float * 3)(*[float(np.float32(v)) for v in d]), (C.c_float * 3)(*[float(v) for v in lum]),
               (C.c_float * 16)(*[float(v) for v in m]), float(bias[0]), float(bias[1]), int(pcf))


HIST_BINS = HISTOGRAM_BINS
