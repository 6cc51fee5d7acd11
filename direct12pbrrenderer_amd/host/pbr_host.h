/* pbr_host.h — C entry points of libpbr_host.so: a small embedding of the C++ pass graph
 * (DeferredRenderPipeline + FrameGraph + RenderScheduler over the HIP kernels) so that tests
 * and tools can drive whole frames through the reference-shaped pass API. */
#ifndef PBR_HOST_H
#define PBR_HOST_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef struct pbrh_renderer pbrh_renderer;

pbrh_renderer* pbrh_create(int hip_device, uint32_t width, uint32_t height, uint32_t env_size, uint32_t lut_res,
                           char* err, size_t err_len);
/* ---- multi-GPU, one renderer per device: this device's tile of a full_w x full_h frame cut cols x rows
 * (rank = row * cols + col; BASELINE cfg5: 7680 x 4320, cols 4, rows 2).  Every target covers the tile's SHADED rectangle;
 * uv / camera ray / ClusterIndex use global pixels, the histogram counts and the tone-map writes the interior only, the
 * average divides by the full frame's pixel count.  halo = 0 (apron mode): the device shades interior + 256 px and blooms
 * that.  halo = 1: it shades interior + 4 px; BloomPass::Execute computes the interior's half-res level, receives the rest
 * of the extended rectangle's half-res level from the neighbouring devices (pbr_halo_exchange over the communicator of
 * pbrh_comm_init) and runs the pyramid on the extended rectangle (pbr_bloom's tiled form). */
pbrh_renderer* pbrh_create_tile(int hip_device, uint32_t full_w, uint32_t full_h, uint32_t cols, uint32_t rows, uint32_t rank, int halo,
                                uint32_t env_size, uint32_t lut_res, char* err, size_t err_len);
/* CPU only: the layout arithmetic behind pbrh_create_tile.  rects = interior, shaded, bloom rectangle (x, y, w, h each, in
 * global pixels); peers = the halo plan, 9 ints per peer: rank, send x y w h, recv x y w h (half-res texels local to the bloom
 * rectangle's half-res plane).  Returns the number of peers, -1 on a bad grid. */
int pbrh_tile_layout(uint32_t full_w, uint32_t full_h, uint32_t cols, uint32_t rows, uint32_t rank, int halo, uint32_t rects[12], int32_t* peers, int max_peers);
/* halo mode without a communicator (several tiles rendered one after the other on ONE device): on = the exchange step only
 * packs the outgoing strips into the renderer's staging area and unpacks whatever the incoming part of it holds;
 * pbrh_halo_copy_from(dst, src) copies the strip src sends to dst into dst's staging area (device to device). */
int pbrh_set_halo_loopback(pbrh_renderer* r, int on);
int pbrh_halo_copy_from(pbrh_renderer* dst, pbrh_renderer* src);
/* 1 (default) = the reference's frame loop: every frame ends with the fence wait (D3D12Device.cpp:993-1003).  k > 1 =
 * throughput mode: a frame's end waits for frame i - k + 1 only, so the host records ahead of the GPU. */
int pbrh_set_frames_in_flight(pbrh_renderer* r, int k);
/* throughput mode only (after pbrh_set_frames_in_flight(k > 1)): a frame's tail — histogram all-reduce, average, tone-map — on
 * the context's high-priority side stream, beside the next frame's cluster pass and shade; the HDR target and the histogram are
 * double-buffered.  Same frames as the plain order (pbrh_read waits for everything in flight).
 * on = 1: as described.  on = 2 (frames without a halo exchange: one GPU, apron mode): the side stream takes over at the bloom pass —
 * bloom chain, histogram, average, tone-map run beside the next frame's cluster pass and shade.  0: off. */
int pbrh_set_tail_overlap(pbrh_renderer* r, int on);
void pbrh_destroy(pbrh_renderer* r);
const char* pbrh_last_error(const pbrh_renderer* r);
/* fp32 RGBA cube mip 0 (host, 6*size*size*4 floats): uploaded, box mips + SH9 computed on the GPU */
int pbrh_set_skybox(pbrh_renderer* r, const float* cube_mip0, uint32_t size);
/* LoadCubeMap: <dir>/{px,nx,py,ny,pz,nz}.hdr (Radiance RGBE) -> sky cube + mips + SH9 on the GPU */
int pbrh_load_skybox(pbrh_renderer* r, const char* dir);
/* pbrh_load_skybox for ONE equirectangular .hdr: resampled into an fp32 cube of `size` with samples^2 sub-samples a texel
 * (pbr_equirect_to_cube on the file's RGBE texels; 0 = the default rule for either), then box mips + SH9 on the GPU */
int pbrh_load_skybox_equirect(pbrh_renderer* r, const char* hdr_path, uint32_t size, uint32_t samples);
/* The reference's own sky asset: a CubeMapResource's data file held in memory (pbrh_parse_cubemap_file describes the layout).  The
 * file is uploaded as it is — 1 byte per texel instead of the 16 of pbrh_set_skybox — and its six BC6H_UF16 chains are decoded in
 * place on the renderer's context (pbr_bc6h_decode_cube) into the sky cube, with the file's own levels (no box mips are made).
 * SkyBoxSH is the file's pack, as the reference takes it (ResourceDef.cpp:211); recompute_sh != 0: pbr_sh9_project of the decoded
 * level 0 instead.  pbrh_load_skybox_file reads the file from disk first. */
int pbrh_set_skybox_file(pbrh_renderer* r, const uint8_t* file, size_t bytes, int recompute_sh);
int pbrh_load_skybox_file(pbrh_renderer* r, const char* path, int recompute_sh);
/* The same file kept RESIDENT: the uploaded bytes are the renderer's sky, the sky pass samples their BC6H blocks in place
 * (pbr_skybox_bc6h) and writes the bits it writes from the decoded cube.  No 16-byte-per-texel cube outlives a call: the prefilter pass
 * decodes into a buffer it releases once its commands are done (once per sky), recompute_sh decodes level 0 into a transient one. */
int pbrh_set_skybox_file_resident(pbrh_renderer* r, const uint8_t* file, size_t bytes, int recompute_sh);
int pbrh_load_skybox_file_resident(pbrh_renderer* r, const char* path, int recompute_sh);
/* the device bytes the renderer holds for its sky: the decoded cube's (16 * pbr_cube_texels) or the resident file's; 0 without a sky */
size_t pbrh_sky_resident_bytes(const pbrh_renderer* r);
/* CPU only, stateless: a serialized CubeMapTextureData (ReflectionDef.h:81-84) held in memory: six faces, each TextureInfo (uint16
 * width, height, depth, mips; uint8 DXGI format; 3 pad bytes), a uint32 payload byte count and the payload (the face's mip chain
 * as BC6H_UF16 blocks: pbr_bc6h_chain_bytes), then SH2CoefficientsPack as 28 floats in pbr_sh_pack's order.  Fills *size, *mips,
 * face_offsets (the byte offset of each face's payload in the file, a multiple of 16) and sh_pack; any of them may be NULL.
 * Returns 0, or -1 + reason in err with nothing written: a truncated file, faces whose TextureInfo differ, width != height,
 * depth != 1, a format outside the reference's HDR range (DXGI 1 .. 18, TextureCompression.cpp:6-10), a byte count that
 * disagrees with pbr_bc6h_chain_bytes or with the file's size. */
int pbrh_parse_cubemap_file(const uint8_t* file, size_t bytes, uint32_t* size, uint32_t* mips, size_t face_offsets[6], float sh_pack[28],
                            char* err, size_t err_len);
/* CPU only, stateless: the inverse.  faces = six HOST chains of pbr_bc6h_chain_bytes(size, mip_levels) bytes in the reference's
 * order px, nx, py, ny, pz, nz; format = the DXGI number written into every TextureInfo (1 .. 18; the reference's skies are
 * R32G32B32A32_FLOAT, 2).  Returns the file's byte count (file NULL: the size needed, nothing read or written), or -1 + reason in
 * err with nothing written: a size or level count pbr_bc6h_chain_bytes rejects, a format outside the HDR range, a null face or
 * pack, file_bytes too small. */
long pbrh_write_cubemap_file(const void* const faces[6], uint32_t size, uint32_t mip_levels, uint32_t format, const float sh_pack[28],
                             uint8_t* file, size_t file_bytes, char* err, size_t err_len);
/* The reference's ResourceLoader::ImportCubeMap (ResourceLoader.cpp:279-299) from decoded faces on: cube_mip0 (host, 6 * size * size
 * fp32 RGBA texels, faces px, nx, py, ny, pz, nz) is uploaded and, on the renderer's context and in this order, its box mips are
 * made (pbr_cube_gen_mips), the SH pack projected from the fp32 level 0 — BEFORE compression, where the reference computes it
 * (BasicStorage.h:313), not from the decoded blocks — and the chain compressed (pbr_bc6h_encode_cube); the blocks are read back
 * and written by pbrh_write_cubemap_file with format 2.  pbrh_import_cubemap_dir takes <dir>/{px,nx,py,ny,pz,nz}.hdr instead
 * (pbrh_load_skybox's parse and pbr_rgbe_decode).  mip_levels 0 = the full chain.  Returns the file's byte count — file_out NULL:
 * the size needed, and nothing runs on the GPU (the _dir form still reads the six files, for their size) — or -1 + reason in err:
 * a size or level count pbr_bc6h_chain_bytes rejects, a null level 0, file_bytes too small, an unreadable or unequal face.
 * What it writes goes to pbrh_set_skybox_file / pbrh_load_skybox_file as it is. */
long pbrh_import_cubemap(pbrh_renderer* r, const float* cube_mip0, uint32_t size, uint32_t mip_levels,
                         uint8_t* file_out, size_t file_bytes, char* err, size_t err_len);
long pbrh_import_cubemap_dir(pbrh_renderer* r, const char* dir, uint32_t mip_levels,
                             uint8_t* file_out, size_t file_bytes, char* err, size_t err_len);
/* The same two with the flags of pbr_bc6h_encode_cube_ex: 0 is the call above, PBR_BC6H_ENCODE_TWO_REGION lets the compression use
 * the ten two-region modes as well (an ordinary cube-map file either way: every reader decodes all fourteen modes); any other bit
 * is refused, the size query included. */
long pbrh_import_cubemap_ex(pbrh_renderer* r, const float* cube_mip0, uint32_t size, uint32_t mip_levels, uint32_t flags,
                            uint8_t* file_out, size_t file_bytes, char* err, size_t err_len);
long pbrh_import_cubemap_dir_ex(pbrh_renderer* r, const char* dir, uint32_t mip_levels, uint32_t flags,
                                uint8_t* file_out, size_t file_bytes, char* err, size_t err_len);
/* The same import from ONE equirectangular (latitude-longitude) panorama instead of six faces — not the reference's, which takes
 * faces only: level 0 is resampled on the GPU by pbr_equirect_to_cube (its rule: include/pbr_hip.h) into a cube of `size` with
 * samples^2 sub-samples a texel, and everything after level 0 is pbrh_import_cubemap_dir_ex's: the same mips, SH pack, flags, file
 * and size query by a NULL file_out.  size 0 / samples 0: the default rules (pbr_equirect_default_size / _samples of the panorama's
 * width).  _equirect takes pano, host fp32 RGBA, ph rows of pw texels, row 0 the top (the size query reads pw only: pano may be
 * NULL); _hdr takes one Radiance .hdr file of any aspect ratio, whose RGBE texels are uploaded as they are (4 bytes a texel) and
 * decoded where the kernel fetches them (the size query still reads the file, for its width).  -1 + reason in err: what the import
 * above refuses, a panorama above PBR_EQUIRECT_MAX_W x PBR_EQUIRECT_MAX_H, samples not 0, 1, 2, 4 or 8, an unreadable file. */
long pbrh_import_cubemap_equirect(pbrh_renderer* r, const float* pano, uint32_t pw, uint32_t ph, uint32_t size, uint32_t samples,
                                  uint32_t mip_levels, uint32_t flags, uint8_t* file_out, size_t file_bytes, char* err, size_t err_len);
long pbrh_import_cubemap_hdr(pbrh_renderer* r, const char* hdr_path, uint32_t size, uint32_t samples, uint32_t mip_levels, uint32_t flags,
                             uint8_t* file_out, size_t file_bytes, char* err, size_t err_len);
/* CPU only: parse one .hdr file held in memory (header + flat / run-length scanlines) into RGBE texels */
int pbrh_parse_hdr(const uint8_t* file, size_t bytes, uint32_t* w, uint32_t* h, uint8_t* rgbe, size_t rgbe_bytes, char* err, size_t err_len);
/* CPU only, stateless: one of the reference's serialized 2D textures (a texture asset's _data.bin) held in memory: TextureInfo (uint16
 * width, height, depth, mips; uint8 DXGI format; 3 pad bytes), a uint32 payload byte count at offset 12, the payload (the chain
 * as BC1 blocks) at offset 16.  *texture (a pbr_texture2d, 24 B) = the description with format = the stored format |
 * PBR_TEX_BC1_BLOCKS and texels = blocks; the payload is copied to blocks (blocks_bytes >= pbr_texture2d_bytes of the
 * description; blocks NULL: the description only, texels NULL).  What it fills goes to pbr_raster_desc.textures /
 * pbrh_set_textured_meshes as it is, or through pbr_bc1_decode.  Returns 0, or -1 + reason in err with nothing written: a
 * truncated file, a byte count that disagrees with pbr_texture2d_bytes or the file's size, depth != 1, an unknown format, a
 * buffer too small. */
int pbrh_parse_texture_file(const uint8_t* file, size_t bytes, void* texture, void* blocks, size_t blocks_bytes, char* err, size_t err_len);
/* CPU only, stateless: the inverse of pbrh_parse_texture_file, the file half of TextureData::BinarySerialize.  texture = a
 * pbr_texture2d whose format holds PBR_TEX_BC1_BLOCKS and whose texels point to the chain's blocks on the HOST; file receives
 * TextureInfo (uint16 width, height, depth 1, mips; uint8 stored format; 3 zero bytes), the uint32 byte count at offset 12 and
 * the payload at 16.  Returns the file's byte count (file NULL: the size needed, nothing read or written), or -1 + reason in err
 * with nothing written: a description without the flag or one pbr_texture2d_bytes rejects, null blocks, file_bytes too small. */
long pbrh_write_texture_file(const void* texture, uint8_t* file, size_t file_bytes, char* err, size_t err_len);
/* The reference's ResourceLoader::ImportTexture from decoded pixels on (image decoding stays outside): level0 (host, width x height
 * texels of stored_format, one of the four PBR_TEX_* formats) is uploaded, its chain of mip_levels levels made by
 * pbr_texture2d_gen_mips and compressed by pbr_bc1_encode on the renderer's context, read back and written to file_out by
 * pbrh_write_texture_file.  Returns the file's byte count (file_out NULL: the size needed, nothing runs), or -1 + reason in err.
 * Like the reference (ResourceLoader.cpp:363-367) it refuses a level 0 whose width or height is not a multiple of 4. */
long pbrh_import_texture(pbrh_renderer* r, const void* level0, uint32_t width, uint32_t height, uint32_t stored_format, uint32_t mip_levels,
                         uint8_t* file_out, size_t file_bytes, char* err, size_t err_len);
/* n lights: position[3], color[3], radius, intensity (8 floats each) */
int pbrh_set_lights(pbrh_renderer* r, const float* lights, int n);
/* the "mSceneLight" records of a reference scene file (Asset/Scene/main.json: Scene.h:192, ReflectionDef.h:119-149) replace
 * the renderer's lights, in file order (Scene::PostDeserialized, Scene.cpp:83-99) */
int pbrh_load_scene_lights(pbrh_renderer* r, const char* scene_json_path);
/* CPU only: the same records of a scene file held in memory as 8-float records (as pbrh_set_lights takes them); returns the
 * count (may exceed max_lights), -1 + reason in err on malformed input */
int pbrh_parse_scene_lights(const char* json, size_t bytes, float* lights, int max_lights, char* err, size_t err_len);
int pbrh_set_gbuffer(pbrh_renderer* r, const uint32_t* A, const uint32_t* B, const uint32_t* C, const float* depth, const uint8_t* stencil);
/* alternative to pbrh_set_gbuffer: the rasterizer's per-pixel material attributes (three float4 planes, see
 * pbr_gbuffer_encode in pbr_hip.h); GBufferPass encodes them on the GPU */
int pbrh_set_materials(pbrh_renderer* r, const float* m0, const float* m1, const float* m2, const float* depth, const uint8_t* stencil);
/* constant-material triangle meshes instead of planes: n_vertices pbr_vertex (56 B), n_indices uint32 indices and n_draws pbr_draw
 * (164 B; include/pbr_hip.h), host arrays copied here and uploaded once by GBufferPass, which then rasterizes them every frame
 * (pbr_gbuffer_raster, draws in the order given) into GBufferA/B/C and GBufferDepthStencil.  pbrh_set_gbuffer / pbrh_set_materials
 * drop the meshes again. */
int pbrh_set_meshes(pbrh_renderer* r, const void* vertices, uint32_t n_vertices, const uint32_t* indices, uint32_t n_indices,
                    const void* draws, uint32_t n_draws);
/* pbrh_set_meshes plus textures: maps = n_draws pbr_draw_maps (20 B), textures = n_textures descriptors whose `texels` point to
 * HOST chains in the reference's layout (pbr_texture2d records, include/pbr_hip.h).  Everything is copied here; GBufferPass uploads the
 * chains once after each change and rasterizes through pbr_gbuffer_raster with maps. */
int pbrh_set_textured_meshes(pbrh_renderer* r, const void* vertices, uint32_t n_vertices, const uint32_t* indices, uint32_t n_indices,
                             const void* draws, uint32_t n_draws, const void* maps, const void* textures, uint32_t n_textures);
/* Scene::CullModel for the meshes (default off): GBufferPass computes the draws' bounds on the GPU when it uploads the meshes
 * (pbr_draw_bounds) and rasterizes through pbr_gbuffer_raster with bounds: draws outside the
 * target's frustum are not set up; the frame is bit-identical.  Works with pbrh_set_meshes and pbrh_set_textured_meshes, before or
 * after them. */
int pbrh_set_model_culling(pbrh_renderer* r, int on);
/* GBufferPass's mCullingStatus of the last frame rendered with culling on: out = {NumDrawCall, NumCulled, triangles drawn, triangles
 * culled} (zeros with culling off).  The copy and the synchronisation happen here, not per frame. */
int pbrh_culling_status(pbrh_renderer* r, uint32_t out[4]);
int pbrh_set_initial_luminance(pbrh_renderer* r, float v);
/* ---- multi-GPU: this renderer's target is the apron-extended tile at (x0, y0) of a full_w x full_h frame;
 * it OWNS the interior rectangle (ix, iy, iw, ih) of its target.  uv / camera ray / ClusterIndex use global pixels, the
 * camera's aspect ratio is the full frame's, the histogram counts and the tone-map writes the interior only, and the
 * average divides by the full frame's pixel count. */
int pbrh_set_tile(pbrh_renderer* r, uint32_t x0, uint32_t y0, uint32_t full_w, uint32_t full_h,
                  uint32_t ix, uint32_t iy, uint32_t iw, uint32_t ih);
/* one process per GPU: RCCL communicator of the context (unique id from pbr_comm_unique_id on rank 0); the average
 * pass then all-reduces the 256-bin histogram (pbr_allreduce_hist) */
int pbrh_comm_init(pbrh_renderer* r, int world, int rank, const void* unique_id_128_bytes);
/* no communicator (tiles rendered one after the other on one device, or a host that moves the 1 KiB itself): the
 * other tiles' counts, added before the average (NULL: none); and a host copy of this tile's own counts */
int pbrh_set_external_histogram(pbrh_renderer* r, const uint32_t* counts256);
int pbrh_capture_histogram(pbrh_renderer* r, int on);
int pbrh_captured_histogram(pbrh_renderer* r, uint32_t* dst256);
/* on: ClusteredPass, BloomPass and the one-shot PreFilterEnvMapPass hand their fixed dispatch sequences over as one call each
 * (pbr_clustered, pbr_bloom, pbr_prefilter_env); off (default): every reference dispatch is issued one by one.
 * The per-frame passes give the same frame bit for bit either way; the fused env chain is within 1 fp16 ULP of the five
 * dispatches (tests/test_host_graph.py).  May be switched between frames. */
int pbrh_set_fused(pbrh_renderer* r, int on);
/* Anti-aliasing (not in the reference): on adds AntiAliasPass (pbr_fxaa, the integer edge filter of include/pbr_hip.h) between
 * ToneMapping and Present; it writes the frame-graph texture "AntiAliasedTexture" (RGBA8, readable through pbrh_read), which becomes
 * the presented one, and ToneMappedTexture stays what it is.  Off by default; off, the execution order, the dispatch count and every
 * resource are those of a renderer that never heard of it.  -1 for a renderer made by pbrh_create_tile or given pbrh_set_tile (the
 * filter reads 25 pixels beyond a tile) and while the overlapped tail is on. */
int pbrh_set_antialiasing(pbrh_renderer* r, int on);
/* Sun light with a shadow map (not in the reference, which computes a directional light and never adds it): SunLightPass (pbr_sun_light
 * of include/pbr_hip.h) between DeferredShading (and the sky resolve) and Bloom, adding into DeferredShadingRT; with shadows != 0 also
 * SunShadowPass after GBuffer, which needs pbrh_set_meshes: it fits the light's orthographic camera (pbr_sun_fit) around the union of
 * the draws' world boxes and rasterizes the meshes (pbr_gbuffer_raster, the constant-material call) into the frame-graph texture
 * "SunShadowDepth" (map_size^2, D32 readable through pbrh_read) — once per mesh upload / pbrh_set_sun_light, not per frame; 17 B per
 * texel with the scratch planes it ignores, 71 MB at 2048^2 (pbrh_set_sun_shadow_depth_only, below: 4 B per texel, the same bits).  dir: world space, from the surface towards the light (normalised here);
 * luminance: three channels; pcf 1 or 3; the biases in light-clip depth units (DeferredFrame.SUN_BIAS of the Python side: 5e-4, 4e-3).
 * Off by default; off, and after pbrh_clear_sun_light, the execution order, the dispatch count and the resources are those of a
 * renderer that never heard of it.  -1: a renderer made by pbrh_create_tile or given pbrh_set_tile — the kernel takes a tile and a
 * tile would be bit-identical to the frame, but every device would rasterize the whole map and nothing here verifies that
 * arrangement, so it is refused rather than left untested —, an overlapped tail, pcf not 1 or 3, a map size outside
 * [3, PBR_RASTER_MAX_SIZE], non-finite arguments, a zero direction.  A refused call changes nothing: a sun set by an earlier call stays
 * as it was, with its map.  A shadowed sun without meshes fails at the next pbrh_render.  SunShadowDepth always has the size of the
 * last successful call; pbrh_clear_sun_light and a sun without shadows free it (and the pass's scratch planes). */
int pbrh_set_sun_light(pbrh_renderer* r, const float dir[3], const float luminance[3], uint32_t map_size, uint32_t pcf, float bias_const,
                       float bias_slope, int shadows);
int pbrh_clear_sun_light(pbrh_renderer* r);
/* The shadow pass of every sun set AFTER this call (pbrh_set_sun_light reads the switch; a sun already set keeps its pass): on != 0,
 * SunShadowPass rasterizes the map with pbr_depth_raster instead of pbr_gbuffer_raster — still one dispatch, the same pass order and
 * dispatch count, "SunShadowDepth" with the same name, size and depth bits (pbr_depth_raster's contract) —, without the three
 * map-sized scratch planes and on the depth raster's smaller scratch: 4 B per texel written instead of 17.  The texture's stencil
 * plane is then not written.  Off by default.  -1 for a null renderer only. */
int pbrh_set_sun_shadow_depth_only(pbrh_renderer* r, int on);
/* the name of the frame-graph texture the present pass shows ("ToneMappedTexture"; "AntiAliasedTexture" with anti-aliasing on) */
int pbrh_presented(pbrh_renderer* r, char* buf, size_t len);
/* n frames; *ms_per_frame = average wall time per frame (every frame ends with the per-frame fence wait) */
int pbrh_render_n(pbrh_renderer* r, int n, float delta_time, double* ms_per_frame);
/* one frame through RenderScheduler::ExecutePipeline; blocks until the GPU is done */
int pbrh_render(pbrh_renderer* r, float delta_time);
/* "PreFilterEnvMap>PrecomputeBRDF>..." */
int pbrh_execution_order(pbrh_renderer* r, char* buf, size_t len);
int pbrh_dispatch_count(const pbrh_renderer* r);
/* the named ranges (the reference's PIXScope strings; roctx ranges here) the last frame opened, '>'-separated, in order */
int pbrh_event_log(const pbrh_renderer* r, char* buf, size_t len);
/* copy a frame-graph resource (by its FGResourceIDs name) to host memory; returns bytes copied or <0 */
long pbrh_read(pbrh_renderer* r, const char* resource_name, void* dst, size_t dst_bytes);
/* the global constants the last frame used (412 bytes) */
int pbrh_get_global(const pbrh_renderer* r, void* dst_412_bytes);
/* builds DeferredRenderPipeline + FrameGraph without touching a GPU and returns the sorted pass order */
/* CPU only (no device): which of the n lights (8 floats each, as pbrh_set_lights) Scene::CullLight hands to the
 * light buffer for the reference camera at cam_pos_yaw = (x, y, z, yaw), and in what order; returns the count
 * (may exceed max_indices), -1 if a light's culling bound leaves the world box */
int pbrh_cull_lights(uint32_t width, uint32_t height, const float cam_pos_yaw[4], const float* lights, int n, int* indices, int max_indices);
/* CPU only: the PointLight[] (pbr_light, 44 bytes each) ClusteredPass::Execute commits for these lights and that camera
 * (DeferredPipeline.cpp:224-241): cull membership + order, attenuation presets (Scene.cpp:132-165); count, or -1 */
int pbrh_light_buffer(uint32_t width, uint32_t height, const float cam_pos_yaw[4], const float* lights, int n, void* out_pbr_lights, int capacity);
/* CPU only: the scene file's lights through Scene::PostDeserialized (AddSceneLights) and Scene::CullLight for the reference default
 * camera moved / rotated as given: bounds6[i] = world AABB {min xyz, max xyz} of light i as the cull sees it (SceneObject::GetWorldBound:
 * the object's matrix — FromEulerAngle(mRotation in degrees), SetScale, translation — applied to the two corners of the local cube,
 * MathLib.cpp:5-10), visible[k] = indices in visiting order.  Returns the number of lights (<= max_lights filled), *n_visible the number
 * visited; -1 + reason on malformed input. */
int pbrh_scene_light_bounds(uint32_t width, uint32_t height, const float cam_pos_yaw[4], const char* json, size_t bytes,
                            float* bounds6, int max_lights, int* visible, int* n_visible, char* err, size_t err_len);
int pbrh_dry_run_execution_order(uint32_t width, uint32_t height, char* buf, size_t len);
/* ShadingState contract probes (no GPU work): 1 = the call returned true */
int pbrh_probe_binding(const char* shader_file, int is_compute, const char* semantic_name, int kind);
#ifdef __cplusplus
}
#endif
#endif
