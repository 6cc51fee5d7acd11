"""pbr_fxaa / pbr_fxaa_batch on the GPU (include/pbr_hip.h, "Anti-aliasing"): every comparison is exact equality with the restatement
tests/fxaa_ref.py.  Sizes around the kernel's 64 x 16 tile, pitches and pointer offsets that take the 16-byte and the 4-byte access
paths, sentinel guards around both images, translation across tiles, batches against their single calls, refusals, and the frames
(DeferredFrame, MultiViewFrame, the C++ host graph) that run the pass behind their tone-map."""
import os

import numpy as np
import pytest
import torch

import common
import fxaa_cases as cases
import fxaa_ref as ref
from direct12pbrrenderer_amd import scene
from direct12pbrrenderer_amd.api import PbrError
from direct12pbrrenderer_amd.structs import MAX_VIEWS

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
TILE_W, TILE_H = 64, 16          # k_fxaa's block tile (csrc/fxaa.hip)


class Padded:
    """an image inside a sentinel-filled device buffer: `rows` guard rows above and below, x0 guard columns to its left, the rest of
    the pitch to its right"""

    def __init__(self, ctx, w, h, pitch, x0=0, rows=2, img=None):
        assert pitch >= x0 + w
        self.w, self.h, self.pitch, self.x0, self.rows = w, h, pitch, x0, rows
        host = np.full((h + 2 * rows, pitch), GUARD, dtype=np.uint32)
        if img is not None:
            host[rows:rows + h, x0:x0 + w] = img
        self.host = host
        self.dev = ctx.upload(host.view(np.int32))
        self.ptr = self.dev.data_ptr() + 4 * (rows * pitch + x0)

    def read(self):
        """-> (the image, everything else as a flat array)"""
        a = self.dev.cpu().numpy().view(np.uint32)
        inside = np.zeros(a.shape, dtype=bool)
        inside[self.rows:self.rows + self.h, self.x0:self.x0 + self.w] = True
        return a[self.rows:self.rows + self.h, self.x0:self.x0 + self.w].copy(), a[~inside]


def run(ctx, img, src_pitch=None, dst_pitch=None, sx0=0, dx0=0):
    """filter img through guarded buffers; asserts the guards and the source unchanged; -> the filtered image"""
    h, w = img.shape
    src = Padded(ctx, w, h, src_pitch or w + sx0, sx0, img=img)
    dst = Padded(ctx, w, h, dst_pitch or w + dx0, dx0)
    ctx.fxaa(src.ptr, w, h, src.pitch, dst.ptr, dst.pitch)
    ctx.sync()
    out, around = dst.read()
    assert (around == GUARD).all(), "a write outside the destination image"
    assert np.array_equal(src.dev.cpu().numpy().view(np.uint32), src.host), "the source changed"
    return out


_REF = {}


def expect(key, img):
    """the restatement of img, computed once per key"""
    if key not in _REF:
        _REF[key] = ref.fxaa(img)
    return _REF[key]


SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3)] + [(w, h) for w in (TILE_W - 1, TILE_W, TILE_W + 1) for h in (TILE_H - 1, TILE_H, TILE_H + 1)] + \
        [(2 * TILE_W + 1, 2 * TILE_H + 1), (70, 45), (256, 144)]


@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_sizes_and_pitches(ctx, w, h):
    """noise (every pixel an edge) and blobs at every size: with tight pitches (16-byte accesses where w is a multiple of 4), with
    pitches above w that are multiples of 4 (16-byte accesses, guard columns) and with odd pitches and pointer offsets (4-byte accesses)"""
    for name, img in (("noise", cases.noise(w, h, seed=w * 1000 + h)), ("blobs", cases.blobs(w, h, seed=w + h))):
        want = expect((name, w, h), img)
        assert np.array_equal(run(ctx, img), want), (name, "tight")
        up = (w + 3) // 4 * 4
        assert np.array_equal(run(ctx, img, src_pitch=up + 8, dst_pitch=up + 4), want), (name, "aligned pitches above w")
        assert np.array_equal(run(ctx, img, src_pitch=w + 7, dst_pitch=w + 5, sx0=3, dx0=1), want), (name, "odd pitches and offsets")
        assert np.array_equal(run(ctx, img, src_pitch=up + 8, dst_pitch=w + 5, dx0=2), want), (name, "aligned source, odd destination")


def contents(w, h):
    out = dict(cases.structured(w, h))
    # half-planes through corners of the block tile, shallow and steep, both signs
    for k, (slope, sign) in enumerate(((1 / 3, 1), (1 / 8, -1), (3.0, 1), (16.0, -1))):
        through = (TILE_W * (1 + k % 2), TILE_H * (1 + k))
        out[f"half-plane {slope:.3g} {sign} through {through}"] = cases.half_plane(w, h, slope, sign, 1 / 8, cases.COLOUR_PAIRS[k % 3], through)
    # axis-aligned steps longer than the walk, on a tile boundary and inside a tile; a step that ends inside the image
    out["step on a tile row"] = cases.step(w, h, TILE_H)
    out["step in a tile"] = cases.step(w, h, TILE_H + 5, 10, w - 30)
    out["vertical step on a tile column"] = np.ascontiguousarray(cases.step(h, w, TILE_W).T)
    out["line on the last row of a tile"] = cases.line(w, h, 2 * TILE_H - 1)
    return out


@pytest.mark.parametrize("w,h", [(70, 45), (256, 144)], ids=lambda v: str(v))
def test_contents(ctx, w, h):
    """noise, thresholded blobs, half-planes through tile corners, a one-pixel line, a checkerboard, axis-aligned steps longer than the
    walk, a jog, edges on the frame's border rows and columns"""
    for name, img in contents(w, h).items():
        got = run(ctx, img, src_pitch=w + 8, dst_pitch=w + 4) if w % 4 == 0 else run(ctx, img)
        assert np.array_equal(got, expect(("content", name, w, h), img)), name
    # the long step: both walks run out (the restatement's intermediate values say so; the bytes above are what the kernel is held to)
    d = ref.fxaa(cases.step(w, h, TILE_H), details=True)[1]
    assert (d["kn"][TILE_H, 24:w - 24] == 24).all() and (d["kp"][TILE_H, 24:w - 24] == 24).all()


def test_translation(ctx):
    """one 40 x 24 pattern pasted at a dozen offsets relative to the tile origin inside 256 x 144 (inside one tile column, across two
    tiles, across four and more): the filtered pattern and the two pixels around it are the same bytes at every offset"""
    w, h, pw, ph = 256, 144, 40, 24
    pattern = cases.blobs(pw, ph, seed=5)
    pattern[5, 3:30] = cases.rgba(255, 250, 240, 17)         # a line and a dot on top of the blobs
    pattern[15, 33] = cases.rgba(0, 0, 0, 99)
    offsets = [(TILE_W, TILE_H), (TILE_W - 1, TILE_H - 1), (TILE_W + 1, TILE_H + 1), (3, 3), (12, 2 * TILE_H + 4), (40, 20), (44, 8), (100, 50),
               (2 * TILE_W - 1, 2 * TILE_H - 1), (2 * TILE_W, 4 * TILE_H), (190, 100), (w - pw - 2, h - ph - 2)]
    crops = []
    for ox, oy in offsets:
        img = np.full((h, w), cases.DARK, dtype=np.uint32)
        img[oy:oy + ph, ox:ox + pw] = pattern
        out = run(ctx, img, src_pitch=w + 4, dst_pitch=w)
        crops.append(out[oy - 2:oy + ph + 2, ox - 2:ox + pw + 2])
        rest = out.copy()
        rest[oy - 2:oy + ph + 2, ox - 2:ox + pw + 2] = cases.DARK
        assert (rest == cases.DARK).all(), (ox, oy)
    want = ref.fxaa(np.pad(pattern, 30, constant_values=cases.DARK))[28:-28, 28:-28]
    for (ox, oy), c in zip(offsets, crops):
        assert np.array_equal(c, want), (ox, oy)
    assert (want[2:-2, 2:-2] != pattern).any()


@pytest.mark.parametrize("n,w,h", [(3, 70, 45), (MAX_VIEWS, 256, 144)], ids=lambda v: str(v))
def test_batch_equals_single_calls(ctx, n, w, h):
    """n images of different contents, pitches and alignments in one launch: each destination is bit-identical to its single call's
    (and, for the first three, to the restatement); guards and sources unchanged"""
    kinds = list(contents(w, h).items())
    imgs = [cases.noise(w, h, seed=70 + k) if k % 3 == 0 else kinds[k % len(kinds)][1] for k in range(n)]
    up = (w + 3) // 4 * 4
    srcs = [Padded(ctx, w, h, up + 4 * (k % 3) + (k % 2) * 3, (k % 2) * 3, img=img) for k, img in enumerate(imgs)]
    dsts = [Padded(ctx, w, h, up + 4 * (k % 2) + (k % 3 == 1) * 1, (k % 3 == 1) * 1) for k in range(n)]
    ctx.fxaa_batch([(s.ptr, s.pitch, d.ptr, d.pitch) for s, d in zip(srcs, dsts)], w, h)
    ctx.sync()
    for k, (s, d, img) in enumerate(zip(srcs, dsts, imgs)):
        out, around = d.read()
        assert (around == GUARD).all(), k
        assert np.array_equal(s.dev.cpu().numpy().view(np.uint32), s.host), k
        assert np.array_equal(out, run(ctx, img, src_pitch=s.pitch, dst_pitch=d.pitch, sx0=s.x0, dx0=d.x0)), k
        if k < 3:
            assert np.array_equal(out, ref.fxaa(img)), k


def test_refusals(ctx):
    """every refusal of the header raises and leaves sentinel-filled destinations untouched"""
    w, h = 70, 45
    img = cases.noise(w, h, seed=9)
    src, src2 = Padded(ctx, w, h, 72, img=img), Padded(ctx, w, h, 72, img=img)
    dst, dst2 = Padded(ctx, w, h, 72), Padded(ctx, w, h, 72)
    ok = dict(src=src.ptr, w=w, h=h, src_pitch=72, dst=dst.ptr, dst_pitch=72)
    single = [dict(src=None), dict(dst=None), dict(w=0), dict(h=0), dict(src_pitch=w - 1), dict(dst_pitch=w - 1),
              dict(dst=src.ptr), dict(dst=src.ptr + 4 * (10 * 72 + 5)), dict(src=dst.ptr + 4 * (h - 1) * 72)]
    for bad in single:
        with pytest.raises(PbrError, match="pbr_fxaa"):
            ctx.fxaa(**dict(ok, **bad))
    a, b = (src.ptr, 72, dst.ptr, 72), (src2.ptr, 72, dst2.ptr, 72)
    batches = [[], [a] * (MAX_VIEWS + 1), [a, (src2.ptr, 72, dst.ptr + 4 * 72, 72)], [a, (dst.ptr, 72, dst2.ptr, 72)], [a, (src2.ptr, 72, src.ptr, 72)],
               [a, (None, 72, dst2.ptr, 72)], [a, (src2.ptr, 72, None, 72)], [a, (src2.ptr, w - 1, dst2.ptr, 72)], [a, (src2.ptr, 72, dst2.ptr, w - 1)]]
    for bad in batches:
        with pytest.raises(PbrError, match="pbr_fxaa_batch"):
            ctx.fxaa_batch(bad, w, h)
    for bad_size in ((0, h), (w, 0)):
        with pytest.raises(PbrError, match="pbr_fxaa_batch"):
            ctx.fxaa_batch([a, b], *bad_size)
    ctx.sync()
    for p in (dst, dst2):
        assert (p.dev.cpu().numpy().view(np.uint32) == GUARD).all()
    for p in (src, src2):
        assert np.array_equal(p.dev.cpu().numpy().view(np.uint32), p.host)
    # sources may alias each other: the same image into two destinations
    ctx.fxaa_batch([a, (src.ptr, 72, dst2.ptr, 72)], w, h)
    ctx.sync()
    assert np.array_equal(dst.read()[0], ref.fxaa(img)) and np.array_equal(dst2.read()[0], dst.read()[0])


# ---- frames ------------------------------------------------------------------------------------------------------------------------
W, H = 256, 144


def dev_half(ctx, a):
    return ctx.upload(np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)).view(torch.float16)


def sphere_grid():
    fx = np.load(os.path.join(common.ROOT, "tests", "golden", "sphere_grid.npz"))
    (v, i, d), _ = scene.reference_models(fx)
    rec = common.reference_scene_lights()
    lights = np.concatenate([scene.make_lights(rec["translation"][j], rec["color"][j], rec["radius"][j], rec["intensity"][j])
                             for j in range(len(rec["radius"]))])
    return v, i, d, lights


def silhouette(stencil):
    """pixels whose stencil differs from a 4-neighbour's: where geometry ends"""
    s = stencil > 0
    m = np.zeros_like(s)
    m[1:, :] |= s[1:, :] != s[:-1, :]
    m[:-1, :] |= s[1:, :] != s[:-1, :]
    m[:, 1:] |= s[:, 1:] != s[:, :-1]
    m[:, :-1] |= s[:, 1:] != s[:, :-1]
    return m


def mesh_frame(ctx, orc, yaw=0.0, spec=None):
    from direct12pbrrenderer_amd.pipeline import DeferredFrame, TileSpec
    sky, env, lut, sh = common.small_ibl(orc)
    cam = scene.Camera.reference_default(W, H)
    if yaw:
        cam.rotate(0.0, yaw, 0.0)
    g = scene.make_global(cam, W, H, sh_pack=sh)
    v, i, d, lights = sphere_grid()
    fr = DeferredFrame(ctx, spec or TileSpec(0, 0, W, H, W, H, 0), g, lights, dev_half(ctx, lut), lut.shape[0], dev_half(ctx, env),
                       common.ENV_SIZE, common.ENV_MIPS)
    fr.set_meshes(v, i, d)
    fr.set_prev_luminance(0.18)
    return fr, g, lights, (lut, env)


def test_deferred_frame(ctx, orc):
    """DeferredFrame.render() of the sphere-grid meshes at 256 x 144 with and without antialias=True: ldr is bit-identical in both,
    ldr_aa is the restatement of ldr and differs from it on silhouette pixels; a frame that is a tile of a larger one refuses"""
    from direct12pbrrenderer_amd.pipeline import TileSpec
    plain, *_ = mesh_frame(ctx, orc)
    plain.render()
    aa, *_ = mesh_frame(ctx, orc)
    aa.render(antialias=True)
    ctx.sync()
    ldr = plain.ldr_numpy()
    assert np.array_equal(aa.ldr_numpy(), ldr)
    got = aa.ldr_aa_numpy()
    assert np.array_equal(got, ref.fxaa(ldr))
    sil = silhouette(aa.gb["stencil"].cpu().numpy())
    assert sil.any() and (got != ldr)[sil].any()
    with pytest.raises(ValueError, match="antialias"):
        plain.ldr_aa_numpy()
    tile, *_ = mesh_frame(ctx, orc, spec=TileSpec(0, 0, W // 2, H, W, H, 0))
    with pytest.raises(ValueError, match="tile"):
        tile.antialias()
    with pytest.raises(ValueError, match="tile"):
        tile.render(antialias=True)


def test_multi_view_frame(ctx, orc):
    """three views of the sphere grid (their G-buffers rasterized by DeferredFrames under three cameras) through MultiViewFrame: ldr is
    what it is without the pass, every ldr_aa the restatement of its ldr, differing from it on silhouette pixels"""
    from direct12pbrrenderer_amd.pipeline import MultiViewFrame
    globals_, gbs, lights = [], [], None
    for yaw in (0.0, 0.2, -0.25):
        fr, g, lights, (lut, env) = mesh_frame(ctx, orc, yaw)
        fr.rasterize()
        ctx.sync()
        gb = {k: t.cpu().numpy() for k, t in fr.gb.items()}
        for k in ("A", "B", "C"):
            gb[k] = gb[k].view(np.uint32)
        globals_.append(g)
        gbs.append(gb)

    def frame():
        mv = MultiViewFrame(ctx, W, H, globals_, [lights] * 3, dev_half(ctx, lut), lut.shape[0], dev_half(ctx, env), common.ENV_SIZE, common.ENV_MIPS)
        mv.upload_gbuffers(gbs)
        mv.set_prev_luminance(0.18)
        return mv
    plain, aa = frame(), frame()
    plain.render()
    aa.render(antialias=True)
    ctx.sync()
    for v in range(3):
        ldr = plain.ldr_numpy(v)
        assert np.array_equal(aa.ldr_numpy(v), ldr)
        got = aa.ldr_aa_numpy(v)
        assert np.array_equal(got, ref.fxaa(ldr)), v
        sil = silhouette(gbs[v]["stencil"])
        assert sil.any() and (got != ldr)[sil].any(), v


def test_host_graph(ctx):
    """the C++ pass graph: off (the default), execution order and dispatch count are those of the dry-run graph, and
    AntiAliasedTexture does not exist; on, AntiAlias runs between ToneMapping and Present with one dispatch more, the presented
    texture is AntiAliasedTexture = the restatement of ToneMappedTexture, and every other target is what it was; off again, the
    frame is the first one's.  Tile renderers and the overlapped tail refuse."""
    import ctypes as C
    from direct12pbrrenderer_amd import synth
    from direct12pbrrenderer_amd.host import HostError, HostRenderer
    ENV, LUT = 32, 64
    v, i, d, lights = sphere_grid()

    def order(r):
        buf = C.create_string_buffer(512)
        assert r.lib.pbrh_execution_order(r.h, buf, 512) == 0
        return buf.value.decode()
    r = HostRenderer(0, W, H, ENV, LUT)
    try:
        r.set_skybox(synth.env_cube(ENV), ENV)
        r.set_lights(lights)
        r.set_meshes(v, i, d)
        r.set_initial_luminance(0.18)
        want = C.create_string_buffer(512)
        assert r.lib.pbrh_dry_run_execution_order(W, H, want, 512) == 0
        parent = want.value.decode()
        assert order(r) == parent and r.presented() == "ToneMappedTexture"
        r.render(1.0 / 60.0)                 # the first frame also runs the one-shot IBL passes
        r.set_initial_luminance(0.18)
        r.render(1.0 / 60.0)
        n_off = r.dispatch_count()
        ldr0, hdr0 = r.read("ToneMappedTexture", (H, W), np.uint32), r.read("DeferredShadingRT", (H, W, 4), np.float16)
        with pytest.raises(HostError):
            r.read("AntiAliasedTexture", (H, W), np.uint32)
        r.set_antialiasing(True)
        assert order(r) == parent.replace("ToneMapping>Present", "ToneMapping>AntiAlias>Present") and order(r) != parent
        assert r.presented() == "AntiAliasedTexture"
        r.set_initial_luminance(0.18)
        r.render(1.0 / 60.0)
        assert r.dispatch_count() == n_off + 1
        ldr1 = r.read("ToneMappedTexture", (H, W), np.uint32)
        got = r.read("AntiAliasedTexture", (H, W), np.uint32)
        assert np.array_equal(ldr1, ldr0) and np.array_equal(r.read("DeferredShadingRT", (H, W, 4), np.float16).view(np.uint16), hdr0.view(np.uint16))
        assert np.array_equal(got, ref.fxaa(ldr1)) and (got != ldr1).any()
        with pytest.raises(HostError, match="anti-aliasing"):
            r.set_tail_overlap(1)
        r.set_antialiasing(False)
        assert order(r) == parent and r.presented() == "ToneMappedTexture"
        r.set_initial_luminance(0.18)
        r.render(1.0 / 60.0)
        assert r.dispatch_count() == n_off
        assert np.array_equal(r.read("ToneMappedTexture", (H, W), np.uint32), ldr0)
        r.set_frames_in_flight(2)
        r.set_tail_overlap(1)
        with pytest.raises(HostError, match="overlapped tail"):
            r.set_antialiasing(True)
    finally:
        r.close()
    t = HostRenderer(0, env_size=ENV, lut_res=LUT, tile=(2 * W, H, 2, 1, 0, False))
    try:
        with pytest.raises(HostError, match="tile"):
            t.set_antialiasing(True)
    finally:
        t.close()
