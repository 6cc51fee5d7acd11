"""Per-frame pass sequence of the deferred pipeline for one GPU's tile of a frame.

Order = the order FrameGraph derives from the passes' declared reads/writes
(Engine/Source/Renderer/FrameGraph.cpp:191-250 on Engine/Include/Renderer/Pipeline/DeferredPipeline.h):
Clustered -> DeferredShading -> Bloom -> AutoExposure -> ToneMapping; bloom is applied to the HDR
buffer BEFORE the luminance histogram and the tone-map.

Multi-GPU: a rank owns an interior tile and shades/blooms it plus an apron of
`apron` pixels on every side that has a neighbour, so the interior is what a single GPU would
produce; the only collective is the 256-bin histogram all-reduce between a16 and a17.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from .api import PbrContext, make_sun, sun_fit
from .scene import draw_bounds, world_box
from .structs import (AABB_DTYPE, DRAW_MAPS_DTYPE, ENV_MIPS, HISTOGRAM_BINS, MAX_VIEWS, NO_MAP, TABLES_BUILT_FRAME, TABLES_BUILT_GEOMETRY, GBuffer, Global, Tile, View)

# bloom's cumulative support: a pixel of an interior whose edges are multiples of 16 depends on level-1 texels
# up to 192 full-res pixels outside it, 195 with the prefilter's reads (3 down + 3 up levels of a radius-4
# kernel on a 2x pyramid; 202 / 205 at any alignment: tests/test_bloom_truth_cpu.py derives both from the
# kernels' integer taps); 256 also keeps every mip of the extended tile on the full frame's texel grid
# (multiple of 16 = 2^(BLOOM_MIPS-1)).
DEFAULT_APRON = 256
# halo mode: the bloom prefilter of a half-res texel reads full-res pixels 2x-3 .. 2x+2 (five taps one half-res
# texel apart, each a 2x2 quad: bloom_prefilter.hlsl:17-60), so 4 shaded pixels beyond the interior make the
# interior's level-1 texels exact; everything further out comes from the neighbours' level 1 (halo exchange).
HALO_SHADE_APRON = 4


@dataclass
class TileSpec:
    """Interior tile (x0,y0,w,h) of a full_w x full_h frame plus the two rectangles a rank works on:
    E = interior + `apron` on every side that has a neighbour (clipped to the frame): where the bloom pyramid runs;
    S = interior + `shade_apron` (clipped): what is shaded.  apron mode: S == E (shade_apron = None);
    halo mode: shade_apron = HALO_SHADE_APRON and level 1 of the pyramid outside the interior comes from the
    neighbours (SURVEY 8e option 2)."""
    x0: int
    y0: int
    w: int
    h: int
    full_w: int
    full_h: int
    apron: int = 0
    shade_apron: int = None

    # ---- E: the bloom rectangle
    @property
    def ex0(self):
        return max(self.x0 - self.apron, 0)

    @property
    def ey0(self):
        return max(self.y0 - self.apron, 0)

    @property
    def ex1(self):
        return min(self.x0 + self.w + self.apron, self.full_w)

    @property
    def ey1(self):
        return min(self.y0 + self.h + self.apron, self.full_h)

    @property
    def ew(self):
        return self.ex1 - self.ex0

    @property
    def eh(self):
        return self.ey1 - self.ey0

    @property
    def ix(self):   # interior offset inside E
        return self.x0 - self.ex0

    @property
    def iy(self):
        return self.y0 - self.ey0

    # ---- S: the shaded rectangle
    @property
    def halo(self):
        return self.shade_apron is not None and self.apron > 0

    @property
    def _sa(self):
        return self.shade_apron if self.halo else self.apron

    @property
    def sx0(self):
        return max(self.x0 - self._sa, 0)

    @property
    def sy0(self):
        return max(self.y0 - self._sa, 0)

    @property
    def sx1(self):
        return min(self.x0 + self.w + self._sa, self.full_w)

    @property
    def sy1(self):
        return min(self.y0 + self.h + self._sa, self.full_h)

    @property
    def sw(self):
        return self.sx1 - self.sx0

    @property
    def sh(self):
        return self.sy1 - self.sy0

    @property
    def six(self):   # interior offset inside S
        return self.x0 - self.sx0

    @property
    def siy(self):
        return self.y0 - self.sy0


def parse_layout(text):
    """'RxC' (rows x cols, the way BASELINE cfg5 says "tiled 2x4": 2 rows of 4 tiles) -> (cols, rows)."""
    r, c = text.lower().split("x")
    return int(c), int(r)


def grid_for_world(world, layout=None):
    """Tile grid (cols, rows) for `world` ranks.  layout: explicit (cols, rows); default = the most square
    factorisation with cols >= rows (1x1, 2x1, 3x1, 2x2, 3x2, 4x2 ...): the shorter the shared edges, the
    smaller the apron / halo."""
    if world < 1:
        raise ValueError("world size must be >= 1")
    if layout is not None:
        cols, rows = int(layout[0]), int(layout[1])
        if cols < 1 or rows < 1 or cols * rows != world:
            raise ValueError(f"layout {cols}x{rows} (cols x rows) does not hold {world} ranks")
        return cols, rows
    rows = max(r for r in range(1, int(world ** 0.5) + 1) if world % r == 0)
    return world // rows, rows


def _check_tiling(world, tile_w, tile_h, apron, full_w, full_h):
    if world > 1 and (tile_w % 16 or tile_h % 16 or apron % 16):
        # every bloom mip of the extended tile must sit on the full frame's texel grid (2^(BLOOM_MIPS-1) = 16)
        raise ValueError("tile size and apron must be multiples of 16 for multi-GPU tiling")
    if full_w > 65535 or full_h > 65535:
        raise ValueError("the assembled frame exceeds 65535 pixels on a side")


def tile_for_rank(rank, world, tile_w, tile_h, apron=DEFAULT_APRON, layout=None, halo=False):
    """Weak scaling: every rank owns one tile_w x tile_h tile of a (cols*tile_w) x (rows*tile_h) frame."""
    cols, rows = grid_for_world(world, layout)
    cx, cy = rank % cols, rank // cols
    _check_tiling(world, tile_w, tile_h, apron, cols * tile_w, rows * tile_h)
    multi = world > 1
    return TileSpec(cx * tile_w, cy * tile_h, tile_w, tile_h, cols * tile_w, rows * tile_h, apron if multi else 0,
                    HALO_SHADE_APRON if (halo and multi) else None)


def tile_of_frame(rank, world, frame_w, frame_h, apron=DEFAULT_APRON, layout=None, halo=False):
    """Strong scaling: a frame_w x frame_h frame cut into cols x rows equal tiles (BASELINE cfg5: 7680x4320,
    2 rows x 4 cols of 1920x2160)."""
    cols, rows = grid_for_world(world, layout)
    if frame_w % cols or frame_h % rows:
        raise ValueError(f"{frame_w}x{frame_h} does not split into {cols}x{rows} equal tiles")
    return tile_for_rank(rank, world, frame_w // cols, frame_h // rows, apron, (cols, rows), halo)


def halo_plan(rank, world, specs):
    """Level-1 (half-res) strips rank `rank` exchanges with every other rank, in GLOBAL half-res texel
    coordinates.  specs: the TileSpec of every rank.  Rank r needs level 1 on E_r/2; it computes it on its
    interior I_r/2 and receives (E_r/2 intersect I_n/2) from each rank n — which covers E_r/2 exactly, because the
    interiors partition the frame and E is clipped to it.  Returns [(peer, send_rect, recv_rect)] with rect =
    (x0, y0, x1, y1) or None; both sides derive the same rectangles from the same specs, so no sizes travel."""
    def half(x0, y0, x1, y1):
        return (x0 // 2, y0 // 2, x1 // 2, y1 // 2)

    def isect(a, b):
        r = (max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3]))
        return r if r[0] < r[2] and r[1] < r[3] else None

    me = specs[rank]
    e_me = half(me.ex0, me.ey0, me.ex1, me.ey1)
    i_me = half(me.x0, me.y0, me.x0 + me.w, me.y0 + me.h)
    plan = []
    for n in range(world):
        if n == rank:
            continue
        o = specs[n]
        recv = isect(e_me, half(o.x0, o.y0, o.x0 + o.w, o.y0 + o.h))
        send = isect(half(o.ex0, o.ey0, o.ex1, o.ey1), i_me)
        if recv or send:
            plan.append((n, send, recv))
    return plan


class HaloTransport:
    """How the level-1 strips travel between ranks in halo mode.  `exchange(frame)` is enqueued between
    pbr_bloom_prefilter's rectangles and pbr_bloom's tiled form.
      "capi"  : pbr_halo_exchange — RCCL send/recv on the context's own communicator (pbr_comm_init);
      "torch" : pbr_halo_pack + torch.distributed P2P (RCCL with the nccl backend) + unpack;
      "host"  : like "torch" but through host copies — gloo rehearsals with several ranks on one GPU."""

    def __init__(self, kind, dist=None):
        assert kind in ("capi", "torch", "host")
        self.kind, self.dist = kind, dist

    def begin(self, fr):
        """torch transport only: run the exchange on a torch side stream so that it overlaps what the caller enqueues until
        end() (the capi transport is enqueued on the context's own side stream instead: DeferredFrame.shade_and_bloom_overlapped)."""
        assert self.kind == "torch"
        if not fr.halo_n:
            return
        main = torch.cuda.current_stream(fr.ctx.torch_device)
        if getattr(self, "side", None) is None:
            self.side = torch.cuda.Stream(fr.ctx.torch_device)
        self.side.wait_stream(main)
        with torch.cuda.stream(self.side):
            fr.ctx.bind_torch_stream()
            self.exchange(fr)
        fr.ctx.bind_torch_stream()

    def end(self, fr):
        if fr.halo_n:
            torch.cuda.current_stream(fr.ctx.torch_device).wait_stream(self.side)

    def exchange(self, fr):
        ctx, a1, pitch, rows = fr.ctx, fr.level1, fr.spec.ew // 2, fr.spec.eh // 2
        if not fr.halo_n:
            return
        if self.kind == "capi":
            ctx.halo_exchange(a1, pitch, rows, fr.halo_peers, fr.halo_n, fr.halo_staging)
            return
        dist = self.dist
        ctx.halo_pack(a1, pitch, rows, fr.halo_peers, fr.halo_n, fr.halo_staging, unpack=False)
        ops, off, host = [], 0, self.kind == "host"
        st = fr.halo_staging
        if host:
            ctx.sync()
            st = st.cpu()
        for peer, send, _ in fr.halo_plan_local:
            if send:
                n = send[2] * send[3]
                ops.append(dist.P2POp(dist.isend, st[off:off + n], peer))
                off += n
        for peer, _, recv in fr.halo_plan_local:
            if recv:
                n = recv[2] * recv[3]
                ops.append(dist.P2POp(dist.irecv, st[off:off + n], peer))
                off += n
        for w in dist.batch_isend_irecv(ops):
            w.wait()
        if host:
            fr.halo_staging.copy_(st)
        ctx.halo_pack(a1, pitch, rows, fr.halo_peers, fr.halo_n, fr.halo_staging, unpack=True)


class ResidentSky:
    """A sky cube kept as the reference's cube-map file on the device: `staged` is the uploaded file (kept alive here), `faces` the
    six addresses of its BC6H_UF16 chains in it (px .. nz).  The sky pass samples the blocks in place (PbrContext.skybox_bc6h); the
    load-time consumers (prefilter_env, sh9_project) take decode()'s transient fp32 cube."""

    def __init__(self, staged, faces, size, mips):
        self.staged, self.faces, self.size, self.mips = staged, [int(f) for f in faces], int(size), int(mips)

    def decode(self, ctx):
        """-> a freshly decoded fp32 cube chain (PbrContext.bc6h_decode_cube) that the caller owns"""
        return ctx.bc6h_decode_cube(self.faces, self.size, self.mips)


class DeferredFrame:
    """Owns the device buffers of one rank and runs the per-frame passes through the C ABI."""

    def __init__(self, ctx: PbrContext, spec: TileSpec, g: Global, lights_np, lut, lut_res, env, env_size,
                 env_mips=ENV_MIPS, allreduce=None, sky=None, all_specs=None, rank=0, halo_transport=None, overlap=False, fused_exposure=False):
        """sky: optional (cube tensor fp32 RGBA with mips, size, mips) — resolved on stencil == 0 pixels
        before the shade like the reference's SkyboxPass; without it those pixels keep what the buffer holds.
        Halo mode (spec.halo): all_specs = the TileSpec of every rank, rank = this one, halo_transport = HaloTransport.
        overlap (halo mode): shade the tile's border RING first, start the exchange of its level-1 strips on a side stream
        and shade the CORE while they travel (falls back to the plain sequence when the tile is too small to split)."""
        self.ctx, self.spec, self.g = ctx, spec, g
        self.sky = sky
        self.n_lights = int(len(lights_np))
        self.lights = ctx.upload(lights_np) if self.n_lights else None
        # env: plain prefiltered chain (pbr_prefilter_env); the shade samples its padded copy (one-shot)
        self.lut, self.lut_res, self.env_size, self.env_mips = lut, lut_res, env_size, env_mips
        self.env = ctx.env_pad(env, env_size, env_mips)
        # the shade reads the LUT from its x-folded table (one-shot, like the padded env chain); _lut_folded names the LUT it was made
        # from: a frame whose lut / lut_res is replaced goes back to the sampled LUT until refold_lut()
        self.lut_fold = None
        self.refold_lut()
        self.allreduce = allreduce
        ew, eh = spec.ew, spec.eh
        self.clusters = ctx.alloc_clusters()
        self.hdr = ctx.zeros((spec.sh, spec.sw, 4), torch.float16)   # covers S (== E in apron mode)
        self.chain_a = ctx.alloc_bloom_chain(ew, eh)
        self.chain_b = ctx.alloc_bloom_chain(ew, eh)
        self.hist = ctx.zeros((HISTOGRAM_BINS,), torch.int32)
        self._tail_overlap = False
        self.avg = ctx.zeros((1,), torch.float32)
        # fused_exposure: average + tone-map as ONE launch (pbr_average_tonemap), which reads one histogram / luminance cell and writes
        # the other — the frame alternates two of each; `hist` / `avg` always name the current ones.  Off by default: measured in round 4
        # (tools/frame_ab.py, profiles/r04_g_frame_ab.txt) the launch it saves does not show in the frame (0.4670 / 0.4672 / 0.4680 vs
        # 0.4659 / 0.4682 / 0.4674 ms), so the frame keeps the reference's two dispatches
        self.fused_exposure = fused_exposure
        self._hist_next = ctx.zeros((HISTOGRAM_BINS,), torch.int32)
        self._avg_next = ctx.zeros((1,), torch.float32)
        self.ldr = ctx.zeros((spec.h, spec.w), torch.int32)
        self.ldr_aa = None   # the anti-aliased target: allocated by the first antialias()
        self.gb = None
        self.mesh = None
        self.sun = None               # set_sun: the directional light pass between the shade and the bloom; None = today's frame
        self._sun_map_stale = True
        self._sun_planes = None
        self.tile = Tile(spec.sx0, spec.sy0, spec.sw, spec.sh, spec.full_w, spec.full_h)
        # the shade tables: the geometry half once per spec, the frame half by every clustered(); the folded shade reads its block
        # prologue from them (tabled=False: the folded shade derives it per block, the same bits)
        self.tabled = True
        self.tables_buf, self.tables = ctx.alloc_shade_tables(spec.sw, spec.sh)
        ctx.shade_geometry_tables(self.tile, self.tables)
        self.halo_transport = halo_transport
        if spec.halo:
            assert all_specs is not None and halo_transport is not None, "halo mode needs every rank's TileSpec and a transport"
            from .structs import bloom_level_offset
            o = bloom_level_offset(ew, eh, 1)
            self.level1 = self.chain_a[o:o + (ew // 2) * (eh // 2)]   # level 1 of chain A: the plane the halo fills
            hx, hy = spec.ex0 // 2, spec.ey0 // 2

            def loc(r):   # global half-res rect (x0,y0,x1,y1) -> (x, y, w, h) in the level-1 plane of E
                return None if r is None else (r[0] - hx, r[1] - hy, r[2] - r[0], r[3] - r[1])
            self.halo_plan_local = [(n, loc(snd), loc(rcv)) for n, snd, rcv in halo_plan(rank, len(all_specs), all_specs)]
            self.halo_peers, self.halo_n = ctx.halo_peers(self.halo_plan_local)
            self.halo_staging = ctx.zeros((max(ctx.halo_staging_bytes(self.halo_peers, self.halo_n) // 8, 1), 4), torch.float16)
        self.split = self._ring_core_split() if (spec.halo and overlap) else None

    def _ring_core_split(self):
        """Rectangles of the overlapped halo frame.  The strips a neighbour needs are the interior's level-1 texels within
        128 half-res texels of the shared edge; their prefilter reads full-res pixels up to 256 + 3 px inside the edge.
        Returns (shade_ring, shade_core, l1_ring, l1_core): shade rects in S-local pixels, level-1 rects in half-res texels
        of the S image; ring U core = S resp. interior / 2, disjoint.  None if the tile is too small to be worth it."""
        s = self.spec
        L, R = s.x0 > 0, s.x0 + s.w < s.full_w
        T, B = s.y0 > 0, s.y0 + s.h < s.full_h
        reach = s.apron + 4                                  # 256 + 3, rounded to keep rectangle edges even
        left = s.six + reach if L else 0
        right = (s.sw - s.six - s.w) + reach if R else 0
        top = s.siy + reach if T else 0
        bot = (s.sh - s.siy - s.h) + reach if B else 0
        mid_w, mid_h = s.sw - left - right, s.sh - top - bot
        if mid_w < 256 or mid_h < 64:
            return None
        ring = [r for r in ((0, 0, s.sw, top), (0, s.sh - bot, s.sw, bot), (0, top, left, mid_h), (s.sw - right, top, right, mid_h))
                if r[2] > 0 and r[3] > 0]
        core = (left, top, mid_w, mid_h)
        hb = s.apron // 2
        ox, oy, iw, ih = s.six // 2, s.siy // 2, s.w // 2, s.h // 2
        l, r_, t, b = (hb if L else 0), (hb if R else 0), (hb if T else 0), (hb if B else 0)
        l1_ring = [q for q in ((ox, oy, iw, t), (ox, oy + ih - b, iw, b), (ox, oy + t, l, ih - t - b), (ox + iw - r_, oy + t, r_, ih - t - b))
                   if q[2] > 0 and q[3] > 0]
        l1_core = (ox + l, oy + t, iw - l - r_, ih - t - b)
        return ring, core, l1_ring, l1_core

    def upload_gbuffer(self, gb_np):
        """gb_np: dict of numpy planes covering the SHADED rectangle S (sh x sw; the extended rectangle in apron mode)."""
        assert gb_np["A"].shape == (self.spec.sh, self.spec.sw)
        self.gb = {k: self.ctx.upload(v) for k, v in gb_np.items()}
        self.mesh = None   # uploaded planes replace meshes set before

    def set_meshes(self, vertices, indices, draws, maps=None, textures=None, cull=False, bounds=None):
        """Geometry instead of uploaded planes: host arrays (structs.VERTEX_DTYPE, uint32 indices, structs.DRAW_DTYPE records) are
        uploaded once, and every render() rasterizes them (pbr_gbuffer_raster, draws in array order) into the frame's own G-buffer
        planes of the shaded rectangle S before the cluster, sky and shade passes (until upload_gbuffer replaces them).
        maps (structs.DRAW_MAPS_DTYPE, one per draw) and textures (the (device tensor, structs.Texture2D) pairs of
        PbrContext.upload_texture or bc1_decode, BC1-resident ones included, which the frame holds on to): the draws' texture maps, rasterized by
        pbr_gbuffer_raster's `maps` when any draw has one.  Without them, or with every map NO_MAP, the call is the
        constant-material one.
        cull: every render() culls the draws against the frustum of the shaded rectangle on the device (pbr_gbuffer_raster's
        `bounds`; the G-buffer is bit-identical) and records cull_stats().  bounds: the draws' local boxes
        (structs.AABB_DTYPE, one per draw; every vertex of a draw inside its box); without them pbr_draw_bounds makes them here, once."""
        s, ctx = self.spec, self.ctx
        draws = np.ascontiguousarray(draws)
        n_tris = int((draws["index_count"] // 3).sum())
        textured = maps is not None and bool((np.asarray(maps).view(np.uint32) != NO_MAP).any())
        self.mesh = {"vertices": ctx.upload(vertices), "n_vertices": len(vertices),
                     "indices": ctx.upload(np.ascontiguousarray(indices, dtype=np.uint32)), "n_indices": len(indices),
                     "draws": ctx.upload(draws), "n_draws": len(draws), "max_triangles": n_tris,
                     "scratch": (ctx.alloc_textured_raster_scratch if textured else ctx.alloc_raster_scratch)(s.sw, s.sh, n_tris)}
        # For the sun's light camera (set_sun fits it around the draws' world boxes) the frame keeps REFERENCES to the caller's host
        # arrays — no copy where they already are numpy arrays of the records' types, which is what scene.MeshScene.arrays() hands
        # out — so a frame that never sets a sun holds the caller's arrays alive and nothing more; the world box is computed from
        # them by the first shadowed sun, once per set_meshes (_sun_world_box).
        self.mesh["host"] = (np.asarray(vertices), np.asarray(indices), draws, None if bounds is None else np.asarray(bounds, dtype=AABB_DTYPE))
        self.mesh["world_box"] = None
        self._sun_map_stale = True
        if textured:
            self.mesh["maps"] = ctx.upload(np.ascontiguousarray(maps, dtype=DRAW_MAPS_DTYPE))
            pairs = list(textures or [])
            if not all(isinstance(t, tuple) and len(t) == 2 for t in pairs):
                raise ValueError("set_meshes: textures are (device tensor, Texture2D) pairs (PbrContext.upload_texture)")
            self.mesh["texture_tensors"] = [t[0] for t in pairs]   # the memory the descriptors point into
            self.mesh["textures"] = [t[1] for t in pairs]
        if cull:
            m = self.mesh
            if bounds is None:
                m["bounds"] = ctx.draw_bounds(m["vertices"], m["n_vertices"], m["indices"], m["n_indices"], m["draws"], m["n_draws"])
            else:
                b = np.ascontiguousarray(bounds, dtype=AABB_DTYPE)
                if len(b) != len(draws):
                    raise ValueError("set_meshes: one bound per draw")
                m["bounds"] = ctx.upload(b)
            m["cull_stats"] = ctx.alloc_cull_stats()
        self.gb = self._planes(s.sh, s.sw)

    def _planes(self, h, w):
        """the five planes of an h x w G-buffer, zeroed"""
        z = self.ctx.zeros
        return {"A": z((h, w), torch.int32), "B": z((h, w), torch.int32), "C": z((h, w), torch.int32), "depth": z((h, w), torch.float32),
                "stencil": z((h, w), torch.uint8)}

    def _raster(self, g, tile, gb, pitch, scratch, **optional):
        """pbr_gbuffer_raster of the meshes under camera g into the planes gb; optional: gbuffer_raster's maps, textures, bounds, stats"""
        m = self.mesh
        self.ctx.gbuffer_raster(g, tile, m["vertices"], m["n_vertices"], m["indices"], m["n_indices"], m["draws"], m["n_draws"],
                                m["max_triangles"], gb["A"], gb["B"], gb["C"], gb["depth"], gb["stencil"], pitch, scratch, **optional)

    def rasterize(self):
        m = self.mesh
        self._raster(self.g, self.tile, self.gb, self.spec.sw, m["scratch"], maps=m.get("maps"), textures=m.get("textures"),
                     bounds=m.get("bounds"), stats=m.get("cull_stats"))

    # Default shadow bias (bias_const, bias_slope), in light-clip depth units, for the default 2048^2 map.  A receiver plane tilted by
    # theta against the light changes its light depth by tan(theta) per unit across the map, and pcf 3 compares against taps up to two
    # texels away: acne needs bias > ~1.5 (E / 2048) tan(theta) / span for a fitted box of extent E and depth span `span`.  1 - NdotL
    # grows with the tilt (0.17 at 34 degrees, 0.5 at 60), so the slope term carries most of it and the constant stays small, which
    # keeps peter-panning (bias x span in world units of depth) small on surfaces that face the light.  Looked at on the tests' ground-
    # and-box scene (tests/test_gpu_sun_frame.py: sun 34 degrees off the ground's normal, E = 13.5, span = 9.4) with the float64 rule
    # at a 256^2 map, whose texel is 8 x the default map's: a total bias of 5.4e-3 still leaves acne on 4 314 of 9 377 open ground
    # pixels (vis down to 0.85), 8e-3 leaves none; that is 1.0e-3 at 2048^2.  These defaults give 1.2e-3 there and 2.5e-3 at 60
    # degrees, where the same estimate asks for 2.5e-3; the contact shadow then starts 1 cm from a caster's foot on that scene.
    SUN_BIAS = (5e-4, 4e-3)

    def set_sun(self, direction, luminance=100.0, map_size=2048, pcf=3, bias=SUN_BIAS, shadows=True, depth_map=None, light_view_proj=None,
                depth_only=False):
        """A directional light with a shadow map, added to the HDR target after the shade (and the sky resolve) and before the bloom
        (pbr_sun_light); set_sun(None) switches it off, and without a sun every launch and output bit of the frame is what it was.
        direction: world space, from the surface towards the light (normalised here); luminance: a scalar or three channels (the
        reference's unused directional light is direction (1, 1, 1), 100 nits).  shadows with meshes (set_meshes): the light's
        orthographic camera is fitted (pbr_sun_fit) around the union of the draws' world boxes and the next render() rasterizes the
        map_size^2 shadow map with pbr_gbuffer_raster — once per set_meshes / set_sun, not per frame; refresh_shadow_map() asks for
        it again (moved draws).  The pass writes a map-sized scratch G-buffer whose A / B / C / stencil planes are ignored: 17 bytes
        per texel, 71 MB at 2048^2.  depth_only=True makes the same map, bit for bit, with pbr_depth_raster instead: the depth plane
        alone, 4 bytes per texel (17 MB at 2048^2), and a raster scratch without the 80-byte resolve record per triangle.  Without meshes (uploaded planes) shadows must be False, or the map is handed in: depth_map =
        (device float32 tensor, map_w, map_h, map_pitch) with its light_view_proj (16 floats)."""
        if direction is None:
            self.sun = None
            return
        if self.split is not None:
            raise ValueError("set_sun: the overlapped halo frame interleaves the shade with the bloom; use the plain frame order")
        sun = {"direction": np.asarray(direction, dtype=np.float64), "luminance": luminance, "pcf": int(pcf), "bias": (float(bias[0]), float(bias[1])),
               "map": None, "map_size": int(map_size), "fit": False, "struct": None, "depth_only": bool(depth_only)}
        if depth_map is not None:
            if light_view_proj is None:
                raise ValueError("set_sun: a depth map needs its light_view_proj")
            sun["map"] = tuple(depth_map)
            sun["struct"] = make_sun(sun["direction"], luminance, light_view_proj, sun["bias"], pcf)
        elif shadows:
            if self.mesh is None:
                raise ValueError("set_sun: shadows need meshes (set_meshes) or an explicit depth_map; pass shadows=False for an unshadowed sun")
            sun["fit"] = True
        else:
            sun["struct"] = make_sun(sun["direction"], luminance, None, sun["bias"], pcf)
        self.sun = sun
        self._sun_map_stale = True

    def refresh_shadow_map(self):
        """the next render() rasterizes the sun's shadow map again (the draws moved)"""
        self._sun_map_stale = True

    def shadow_map(self):
        """(depth tensor, map_w, map_h, map_pitch, light_view_proj as 16 floats) of the sun's shadow map as the last sun_light() used
        it; None without a map"""
        if self.sun is None or self.sun["map"] is None:
            return None
        return (*self.sun["map"], list(self.sun["struct"].LightViewProj))

    def shadow_pass(self):
        """fit the light camera around the draws' world boxes and rasterize the shadow map (the unculled constant-material raster)"""
        sun, m, ctx = self.sun, self.mesh, self.ctx
        if m["world_box"] is None:      # once per set_meshes: the host twin of pbr_draw_bounds walks every index
            vertices, indices, draws, bounds = m["host"]
            m["world_box"] = world_box(draws, bounds if bounds is not None else draw_bounds(vertices, indices, draws))
            if m["world_box"] is None:
                raise ValueError("set_sun: the meshes hold no valid triangle to fit the light's camera around")
        box = m["world_box"]
        n = sun["map_size"]
        d = sun["direction"] / np.sqrt(float((sun["direction"] ** 2).sum()))
        light_g, lvp = sun_fit(d.astype(np.float32), box[0], box[1], n, n)
        # the map-sized scratch G-buffer and raster scratch live on the FRAME, keyed by map size and triangle count: another luminance,
        # bias or direction allocates nothing.  A / B / C / stencil and the scratch are kept for the next raster (refresh_shadow_map)
        # (a depth-only sun keeps the depth plane and the depth raster's smaller scratch, nothing else)
        sm, only = self._sun_planes, sun["depth_only"]
        if sm is None or sm["n"] != n or sm["tris"] != m["max_triangles"] or sm["depth_only"] != only:
            if only:
                sm = dict(depth=ctx.empty((n, n), torch.float32), scratch=ctx.alloc_depth_raster_scratch(n, n, m["max_triangles"]))
            else:
                sm = dict(self._planes(n, n), scratch=ctx.alloc_raster_scratch(n, n, m["max_triangles"]))
            sm.update(n=n, tris=m["max_triangles"], depth_only=only)
            self._sun_planes = sm
        if only:
            ctx.depth_raster(light_g, Tile(0, 0, n, n, n, n), m["vertices"], m["n_vertices"], m["indices"], m["n_indices"], m["draws"],
                             m["n_draws"], m["max_triangles"], sm["depth"], n, sm["scratch"])
        else:
            self._raster(light_g, Tile(0, 0, n, n, n, n), sm, n, sm["scratch"])
        sun["light_g"], sun["map"] = light_g, (sm["depth"], n, n, n)
        sun["struct"] = make_sun(sun["direction"], sun["luminance"], lvp, sun["bias"], sun["pcf"])

    def sun_light(self):
        """pbr_sun_light on the shaded rectangle (after shade(), before the bloom); the shadow map first if it is stale"""
        sun, s = self.sun, self.spec
        if sun["fit"] and self._sun_map_stale:
            if self.mesh is None:
                raise ValueError("sun_light: the meshes the shadow map was to be made from were replaced by uploaded planes")
            self.shadow_pass()
        self._sun_map_stale = False
        depth, mw, mh, mp = sun["map"] if sun["map"] is not None else (None, 0, 0, 0)
        self.ctx.sun_light(self.g, self.tile, self.gb, s.sw, sun["struct"], self.hdr, s.sw, depth, mw, mh, mp)

    def cull_stats(self):
        """structs.CullStats of the last render() of meshes set with cull=True (draws drawn / culled, triangles drawn / culled:
        the reference's mCullingStatus); synchronises"""
        if not self.mesh or "cull_stats" not in self.mesh:
            raise ValueError("cull_stats: set_meshes(..., cull=True) first")
        return self.ctx.read_cull_stats(self.mesh["cull_stats"])

    def set_sky_file(self, data, recompute_sh=False, resident=False):
        """The sky from the bytes of the reference's serialized sky cube (host.parse_cubemap_file): the file is uploaded as it is, its
        six BC6H_UF16 chains are decoded on the GPU (PbrContext.bc6h_decode_cube) into the cube the sky pass samples, with the file's
        own levels, and g.SkyBoxSH becomes the file's SH pack (recompute_sh: the projection of the decoded level 0).  The env chain
        the frame was built with is not touched: prefilter it from sky_cube() when it should follow.  Returns the 28 floats.
        resident: the uploaded file stays alive and IS the sky (self.sky: a ResidentSky, the six addresses into it); skybox() samples
        its blocks in place (PbrContext.skybox_bc6h) to the same bits, at 1 byte per texel instead of 16.  No decoded cube outlives
        this call: recompute_sh decodes into a transient cube, projects and releases it."""
        from . import host
        size, mips, offsets, sh = host.parse_cubemap_file(data)
        staged = self.ctx.upload(np.frombuffer(bytes(data), dtype=np.uint8).copy())
        sky = ResidentSky(staged, [staged.data_ptr() + o for o in offsets], size, mips)
        cube = None if resident and not recompute_sh else sky.decode(self.ctx)
        if recompute_sh:
            pack = self.ctx.sh9_project(cube, size, mips)
            self.ctx.sync()
            sh = pack.cpu().numpy()
        else:
            self.ctx.sync()             # `staged` may be released on return
        C.memmove(C.addressof(self.g.SkyBoxSH), np.ascontiguousarray(sh, dtype=np.float32).ctypes.data, 112)
        self.sky = sky if resident else (cube, size, mips)
        return sh

    def sky_cube(self):
        """-> (cube, size, mips): the sky as the fp32 cube chain prefilter_env and sh9_project take.  Of a resident sky a freshly
        decoded cube that the caller owns (nothing here keeps it alive); otherwise the frame's own."""
        if isinstance(self.sky, ResidentSky):
            return self.sky.decode(self.ctx), self.sky.size, self.sky.mips
        return self.sky

    def set_prev_luminance(self, v):
        self.avg.fill_(float(v))

    # interior views (pointer + pitch) of the HDR buffer
    def _hdr_interior_ptr(self):
        s = self.spec
        return self.hdr.data_ptr() + 8 * (s.siy * s.sw + s.six)

    def clustered(self):
        if self.tabled:
            self.ctx.clustered_tables(self.g, self.lights, self.n_lights, self.clusters, self.tables)
        else:
            self.ctx.clustered(self.g, self.lights, self.n_lights, self.clusters)

    def skybox(self):
        s = self.spec
        if isinstance(self.sky, ResidentSky):
            self.ctx.skybox_bc6h(self.g, self.tile, self.sky.faces, self.sky.size, self.sky.mips, self.gb["stencil"], s.sw, self.hdr, s.sw)
            return
        cube, size, mips = self.sky
        self.ctx.skybox(self.g, self.tile, cube, size, mips, self.gb["stencil"], s.sw, self.hdr, s.sw)

    def refold_lut(self):
        """Rebuild the x-folded table from self.lut (after the LUT's texels were rewritten in place or the tensor was replaced)."""
        self.lut_fold = self.ctx.lut_fold_x(self.lut, self.lut_res, out=self.lut_fold if self.lut_fold is not None and self.lut_fold.shape[0] == self.lut_res else None)
        self._lut_folded = (self.lut.data_ptr(), self.lut_res)

    def _shade(self, rects):
        s = self.spec
        folded = self._lut_folded == (self.lut.data_ptr(), self.lut_res)

        def args(lut):
            return (self.g, self.tile, self.gb, s.sw, lut, self.lut_res, self.env, self.env_size, self.env_mips, self.clusters, self.lights,
                    self.n_lights, self.hdr, s.sw)
        # (a shade before the frame's first clustered(), or after its light set was replaced: the folded shade, which derives its prologue)
        if folded and self.tabled and self.tables.built == TABLES_BUILT_FRAME | TABLES_BUILT_GEOMETRY and self.tables.num_lights == self.n_lights:
            self.ctx.deferred_shade_tabled(*args(self.lut_fold), self.tables, rects)
        elif folded:
            self.ctx.deferred_shade_folded(*args(self.lut_fold), rects)
        elif rects is None:
            self.ctx.deferred_shade(*args(self.lut))
        else:
            self.ctx.deferred_shade_rects(*args(self.lut), rects)

    def shade(self):
        self._shade(None)

    def shade_rects(self, rects):
        """The shade on rectangles (x, y, w, h) of the shaded rectangle S, ONE launch (pbr_deferred_shade with a rectangle list)."""
        self._shade(rects)

    def prefilter_l1_rects(self, rects):
        s = self.spec
        self.ctx.bloom_prefilter_rects(self.hdr, s.sw, s.sh, s.sw, self.level1, s.ew // 2, (s.sx0 - s.ex0) // 2, (s.sy0 - s.ey0) // 2, rects)

    def shade_and_bloom_overlapped(self, histogram=True):
        """Halo frame with the exchange hidden behind the core's shade: ring -> strips -> exchange || core -> pyramid
        (two shade launches and two prefilter launches instead of one each)."""
        ring, core, l1_ring, l1_core = self.split
        ctx, tr = self.ctx, self.halo_transport
        if tr.kind == "torch":     # torch's P2P ops follow torch's current stream: plain fork / join around the exchange
            self.shade_rects(ring)
            self.prefilter_l1_rects(l1_ring)
            tr.begin(self)
            self.shade_rects([core])
            tr.end(self)
        else:                      # ring + its strips + the exchange on the context's high-priority side stream,
            ctx.side_begin()       # the core on the main stream at the same time
            self.shade_rects(ring)
            self.prefilter_l1_rects(l1_ring)
            if tr.kind == "host":
                ctx.side_end()     # the host stand-in synchronises the device anyway
                ctx.side_join()
                tr.exchange(self)
            else:
                tr.exchange(self)  # pbr_halo_exchange, enqueued on the side stream
                ctx.side_end()
            self.shade_rects([core])
            ctx.side_join()
        self.prefilter_l1_rects([l1_core])   # reads 3 px into the ring: after the join
        self.halo_pyramid(histogram)

    def bloom(self):
        s = self.spec
        if s.halo:
            self.bloom_halo(histogram=False)
        else:
            self.ctx.bloom(self.hdr, s.ew, s.eh, s.ew, self.chain_a, self.chain_b)

    def histogram(self):
        s = self.spec
        self.ctx.lum_histogram(self._hdr_interior_ptr(), s.w, s.h, s.sw, self.hist)

    # ---- halo mode: prefilter the interior, fetch the rest of level 1 from the neighbours, run levels 1..4 on E
    def halo_prefilter(self):
        s = self.spec
        self.ctx.bloom_prefilter_rect(self.hdr, s.sw, s.sh, s.sw, self.level1, s.ew // 2, (s.sx0 - s.ex0) // 2, (s.sy0 - s.ey0) // 2,
                                      (s.six // 2, s.siy // 2, s.w // 2, s.h // 2))

    def halo_exchange(self):
        self.halo_transport.exchange(self)

    def halo_pyramid(self, histogram=True):
        s = self.spec
        self.ctx.bloom_tiled(self.hdr, s.sw, (s.sx0 - s.ex0, s.sy0 - s.ey0, s.sw, s.sh), s.ew, s.eh, self.chain_a, self.chain_b,
                             (s.ix, s.iy, s.w, s.h), self.hist if histogram else None)

    def bloom_halo(self, histogram=True):
        self.halo_prefilter()
        self.halo_exchange()
        self.halo_pyramid(histogram)

    def bloom_histogram(self):
        """Bloom with the interior-tile luminance histogram accumulated in its final kernel."""
        s = self.spec
        if s.halo:
            self.bloom_halo(histogram=True)
        else:
            self.ctx.bloom_histogram(self.hdr, s.ew, s.eh, s.ew, self.chain_a, self.chain_b, (s.ix, s.iy, s.w, s.h), self.hist)

    def average(self):
        s = self.spec
        self.ctx.lum_average(self.hist, s.full_w * s.full_h, float(self.g.DeltaTime), self.avg)

    def tonemap(self):
        s = self.spec
        self.ctx.tonemap(self._hdr_interior_ptr(), s.w, s.h, s.sw, self.avg, self.ldr, s.w)

    def average_tonemap(self):
        """The frame's last two dispatches as one launch; afterwards `avg` is the new adapted luminance and `hist` the zeroed
        histogram the next frame accumulates into."""
        s = self.spec
        self.ctx.average_tonemap(self.hist, s.full_w * s.full_h, float(self.g.DeltaTime), self.avg, self._avg_next, self._hist_next,
                                 self._hdr_interior_ptr(), s.w, s.h, s.sw, self.ldr, s.w)
        self.avg, self._avg_next = self._avg_next, self.avg
        self.hist, self._hist_next = self._hist_next, self.hist

    def antialias(self):
        """The anti-aliasing pass (pbr_fxaa) on the tone-mapped target: ldr -> ldr_aa, a second RGBA8 target of the same size (read
        it with ldr_aa_numpy()); ldr is not touched.  Whole frames only: the filter of a tile of a larger frame would need an LDR
        apron of 25 pixels from the neighbouring tiles."""
        s = self.spec
        self._whole_frame_or_raise()
        if self.ldr_aa is None:
            self.ldr_aa = self.ctx.zeros((s.h, s.w), torch.int32)
        self.ctx.fxaa(self.ldr, s.w, s.h, s.w, self.ldr_aa, s.w)

    def _whole_frame_or_raise(self):
        s = self.spec
        if (s.x0, s.y0, s.w, s.h) != (0, 0, s.full_w, s.full_h):
            raise ValueError(f"antialias: this frame is the tile ({s.x0}, {s.y0}, {s.w}, {s.h}) of a {s.full_w} x {s.full_h} frame; the filter "
                             "reads up to 25 pixels beyond a tile and runs on whole frames only")

    def exposure_and_tonemap(self):
        if self.fused_exposure:
            self.average_tonemap()
        else:
            self.average()
            self.tonemap()

    def render(self, shade_events=None, antialias=False):
        """One frame: every per-frame dispatch of the reference, in the frame graph's order.
        shade_events: optional list; a (start, end) pair of torch events bracketing the shade launch is appended.
        antialias: antialias() behind the tone-map, on the stream the tone-map ran on; ldr is what it is without."""
        if antialias:
            self._whole_frame_or_raise()
            if self._tail_overlap:
                raise ValueError("render(antialias=True): the overlapped tail tone-maps on the side stream; call antialias() after finish()")
        self._render(shade_events)
        if antialias:
            self.antialias()

    def _render(self, shade_events):
        if self.mesh is not None:
            self.rasterize()
        self.clustered()
        if self.sky is not None:
            self.skybox()
        if self.split is not None:
            e0 = e1 = None
            if shade_events is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            self.shade_and_bloom_overlapped()
            if shade_events is not None:   # brackets shade + bloom here: the two are interleaved
                e1.record()
                shade_events.append((e0, e1))
            if self.allreduce is not None:
                self.allreduce(self.hist)
            self.exposure_and_tonemap()
            return
        if shade_events is None:
            self.shade()
        else:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.shade()
            e1.record()
            shade_events.append((e0, e1))
        if self.sun is not None:
            self.sun_light()
        if self._tail_overlap == "bloom":
            # everything behind the shade — the bloom chain (8 launches, HBM / latency-bound), average, tone-map — on the context's
            # high-priority side stream, beside the NEXT frame's cluster pass and shade (FP32-issue-bound), which write the other
            # HDR / histogram buffer.  The join makes the main stream wait for the side work of the frame BEFORE (it read the HDR
            # buffer the next shade overwrites); the chains and the adapted luminance are touched by the side stream only, in order.
            self.ctx.side_join()
            self.ctx.side_begin()
            self.bloom_histogram()
            if self.allreduce is not None:
                self.allreduce(self.hist)
            self.average()
            self.tonemap()
            self.ctx.side_end()
            self.hdr, self._hdr_alt = self._hdr_alt, self.hdr
            self.hist, self._hist_alt = self._hist_alt, self.hist
            return
        self.bloom_histogram()
        if self._tail_overlap:
            # the frame's tail — histogram all-reduce, average, tone-map — on the context's side stream: the collective's latency
            # and the two small launches run beside the NEXT frame's cluster pass and shade, which write the other HDR /
            # histogram buffer.  The join orders the side work of the frame BEFORE last ahead of this point (long finished).
            self.ctx.side_join()
            self.ctx.side_begin()
            if self.allreduce is not None:
                self.allreduce(self.hist)
            self.average()
            self.tonemap()
            self.ctx.side_end()
            self.hdr, self._hdr_alt = self._hdr_alt, self.hdr
            self.hist, self._hist_alt = self._hist_alt, self.hist
            return
        if self.allreduce is not None:
            self.allreduce(self.hist)
        self.exposure_and_tonemap()

    def enable_tail_overlap(self, capi_allreduce=False, from_bloom=False):
        """Throughput mode: double-buffer the HDR target and the histogram so that a frame's tail — histogram all-reduce, average,
        tone-map; with from_bloom=True the bloom chain as well, i.e. everything behind the shade — runs on the context's side stream
        beside the NEXT frame's cluster pass and shade.  The LDR image of frame i is complete when frame i + 1's tail has been
        joined (or after ctx.sync(), which also waits for the side stream).  With an all-reduce (world > 1) it MUST be one that is
        enqueued on the context's current stream — PbrContext.allreduce_hist, or a stand-in the caller vouches for with
        capi_allreduce=True (tests: a 1-rank communicator); a torch.distributed all-reduce runs on torch's own stream and would
        race with the double-buffered histogram.  from_bloom is for frames without a halo exchange (one GPU, apron mode)."""
        if self.split is not None:
            raise ValueError("tail overlap needs the plain frame order")
        if self.allreduce is not None:
            own = getattr(self.allreduce, "__self__", None) is self.ctx and getattr(self.allreduce, "__name__", "") == "allreduce_hist"
            if not (own or capi_allreduce):
                raise ValueError("tail overlap needs the C ABI's all-reduce (PbrContext.allreduce_hist): it must be enqueued on the context's side stream")
        if from_bloom and self.spec.halo:
            raise ValueError("from_bloom: the halo exchange stays on the frame's stream")
        self._hdr_alt = torch.zeros_like(self.hdr)
        self._hist_alt = torch.zeros_like(self.hist)
        self._tail_overlap = "bloom" if from_bloom else True

    def finish(self):
        """Wait (on the frame's stream) for an overlapped tail still in flight."""
        if self._tail_overlap:
            self.ctx.side_join()

    # ---- read-back helpers for tests ---------------------------------------------------------------
    def hdr_interior(self):
        s = self.spec
        return self.hdr[s.siy:s.siy + s.h, s.six:s.six + s.w].cpu().numpy()

    def ldr_numpy(self):
        return self.ldr.cpu().numpy().view(np.uint32)

    def ldr_aa_numpy(self):
        if self.ldr_aa is None:
            raise ValueError("ldr_aa_numpy: antialias() or render(antialias=True) first")
        return self.ldr_aa.cpu().numpy().view(np.uint32)


class MultiViewFrame:
    """N camera views of one scene, w x h whole frames each, rendered as ONE chain of launches per MAX_VIEWS views (the pbr_*_views
    entry points): clustered -> [sky] -> shade -> bloom + histogram -> average -> tone-map, the frame graph's order.  View v gets the
    bits a DeferredFrame with the same inputs gets.  The views share the LUT, the env chain and the sky's SH pack (globals[v].SkyBoxSH);
    each has its own camera (globals[v], DeltaTime included), light array, G-buffer and targets."""

    def __init__(self, ctx: PbrContext, w, h, globals, lights_per_view, lut, lut_res, env, env_size, env_mips=ENV_MIPS, sky=None):
        """globals: one Global per view; lights_per_view: one LIGHT_DTYPE array per view; env: the plain prefiltered chain (padded
        here once); sky: optional (cube tensor, size, mips) or a ResidentSky (a DeferredFrame's after set_sky_file(resident=True)), resolved per view on stencil == 0 pixels before the shade."""
        if len(globals) != len(lights_per_view) or not globals:
            raise ValueError("one Global and one light array per view")
        self.ctx, self.w, self.h, self.n = ctx, int(w), int(h), len(globals)
        self.sky = sky
        self.lut, self.lut_res, self.env_size, self.env_mips = lut, lut_res, env_size, env_mips
        self.env = ctx.env_pad(env, env_size, env_mips)
        self.n_lights = [int(len(l)) for l in lights_per_view]
        self.lights = [ctx.upload(l) if len(l) else None for l in lights_per_view]
        self.clusters = [ctx.alloc_clusters() for _ in range(self.n)]
        self.hdrs = [ctx.zeros((self.h, self.w, 4), torch.float16) for _ in range(self.n)]
        self.chain_a = [ctx.alloc_bloom_chain(self.w, self.h) for _ in range(self.n)]
        self.chain_b = [ctx.alloc_bloom_chain(self.w, self.h) for _ in range(self.n)]
        self.hist = [ctx.zeros((HISTOGRAM_BINS,), torch.int32) for _ in range(self.n)]
        self.avg = [ctx.zeros((1,), torch.float32) for _ in range(self.n)]
        self.ldr = [ctx.zeros((self.h, self.w), torch.int32) for _ in range(self.n)]
        self.ldr_aa = None   # the anti-aliased targets: allocated by the first antialias()
        self.gb = None
        self.tile = Tile(0, 0, self.w, self.h, self.w, self.h)
        self.globals = list(globals)
        self._batches = None

    def upload_gbuffers(self, gbs):
        """gbs: one dict of numpy planes (h x w) per view."""
        if len(gbs) != self.n:
            raise ValueError(f"{len(gbs)} G-buffers for {self.n} views")
        for gb in gbs:
            assert gb["A"].shape == (self.h, self.w)
        self.gb = [{k: self.ctx.upload(v) for k, v in gb.items()} for gb in gbs]
        self._build()

    def set_globals(self, globals):
        """new cameras / DeltaTime for the following frames"""
        if len(globals) != self.n:
            raise ValueError(f"{len(globals)} cameras for {self.n} views")
        self.globals = list(globals)
        if self.gb is not None:
            self._build()

    def set_prev_luminance(self, values):
        vals = [float(values)] * self.n if np.isscalar(values) else [float(v) for v in values]
        if len(vals) != self.n:
            raise ValueError(f"{len(vals)} luminance values for {self.n} views")
        for a, v in zip(self.avg, vals):
            a.fill_(v)

    def _view(self, v):
        gb = self.gb[v]
        return View(self.globals[v], GBuffer(gb["A"].data_ptr(), gb["B"].data_ptr(), gb["C"].data_ptr(), gb["depth"].data_ptr(),
                                             gb["stencil"].data_ptr(), self.w),
                    self.lights[v].data_ptr() if self.lights[v] is not None else None, self.n_lights[v], self.clusters[v].data_ptr(),
                    self.hdrs[v].data_ptr(), self.w, self.chain_a[v].data_ptr(), self.chain_b[v].data_ptr(), self.hist[v].data_ptr(),
                    self.avg[v].data_ptr(), self.ldr[v].data_ptr(), self.w)

    def _build(self):
        """the View arrays of the calls: MAX_VIEWS views per call"""
        self._batches = []
        for b0 in range(0, self.n, MAX_VIEWS):
            idx = list(range(b0, min(b0 + MAX_VIEWS, self.n)))
            self._batches.append(((View * len(idx))(*[self._view(v) for v in idx]), len(idx), idx))

    # ---- the frame's stages, each one call per MAX_VIEWS views
    def _calls(self):
        if self._batches is None:
            raise RuntimeError("upload_gbuffers() first")
        return self._batches

    def clustered(self):
        for arr, n, _ in self._calls():
            self.ctx.clustered_views(arr, n)

    def skybox(self):
        for arr, n, _ in self._calls():
            if isinstance(self.sky, ResidentSky):
                self.ctx.skybox_bc6h_views(arr, n, self.w, self.h, self.sky.faces, self.sky.size, self.sky.mips)
            else:
                cube, size, mips = self.sky
                self.ctx.skybox_views(arr, n, self.w, self.h, cube, size, mips)

    def shade(self):
        for arr, n, _ in self._calls():
            self.ctx.deferred_shade_views(arr, n, self.w, self.h, self.lut, self.lut_res, self.env, self.env_size, self.env_mips)

    def bloom_histogram(self):
        for arr, n, _ in self._calls():
            self.ctx.bloom_histogram_views(arr, n, self.w, self.h)

    def average(self):
        for arr, n, _ in self._calls():
            self.ctx.lum_average_views(arr, n, self.w * self.h)

    def tonemap(self):
        for arr, n, _ in self._calls():
            self.ctx.tonemap_views(arr, n, self.w, self.h)

    def antialias(self):
        """The anti-aliasing pass on every view's tone-mapped target, ldr[v] -> ldr_aa[v]: one pbr_fxaa_batch call per MAX_VIEWS views"""
        if self.ldr_aa is None:
            self.ldr_aa = [self.ctx.zeros((self.h, self.w), torch.int32) for _ in range(self.n)]
        for b0 in range(0, self.n, MAX_VIEWS):
            self.ctx.fxaa_batch([(self.ldr[v], self.w, self.ldr_aa[v], self.w) for v in range(b0, min(b0 + MAX_VIEWS, self.n))], self.w, self.h)

    def render(self, antialias=False):
        """One frame of every view: clustered -> [sky] -> shade -> bloom + histogram -> average -> tone-map [-> anti-aliasing]."""
        self.clustered()
        if self.sky is not None:
            self.skybox()
        self.shade()
        self.bloom_histogram()
        self.average()
        self.tonemap()
        if antialias:
            self.antialias()

    # ---- read-back helpers for tests
    def hdr(self, v):
        """view v's HDR target (h x w x 4 fp16 device tensor)"""
        return self.hdrs[v]

    def ldr_numpy(self, v):
        return self.ldr[v].cpu().numpy().view(np.uint32)

    def ldr_aa_numpy(self, v):
        if self.ldr_aa is None:
            raise ValueError("ldr_aa_numpy: antialias() or render(antialias=True) first")
        return self.ldr_aa[v].cpu().numpy().view(np.uint32)
