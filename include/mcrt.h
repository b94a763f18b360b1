/* mcrt.h — C ABI of the MI355X-native tile-render hot path.
 *
 * This is the drop-in boundary for the reference's
 *     TileRenderer::render(const Scene&, const RayTracer::Config&, std::function<void(int,int)>)
 *     (/root/reference/src/raytracer/tile_renderer.h:26-28, tile_renderer.cpp:129-189)
 * and everything below it (renderTile → RayTracer::traceRay → intersectScene / shade).
 * Plain C types only: pointers + sizes, caller-owned buffers, no STL, no torch types.
 * The reference-side binding (how `Scene` is turned into `mcrt_scene_desc`) is shown in
 * INTEGRATION.md and shipped as minecraftskin_raytracer_amd/csrc/host/tile_renderer_hip.cpp.
 *
 * Three libraries implement (parts of) this ABI with different prefixes:
 *   libmcrt.so        (product, HIP/gfx950)      mcrt_*        — this header
 *   libmcrt_oracle.so (tests only, CPU)          mcrt_oracle_* — oracle/mcrt_oracle.h
 *   libmcref.so       (tests only, the compiled reference itself, built from /root/reference
 *                      where it lies)            mcref_*       — oracle/ref_shim.cpp
 */
#ifndef MCRT_H
#define MCRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCRT_ABI_VERSION 3 /* 2: mcrt_render_multi, MCRT_DEVICE_ALL; mcrt_time_render_device lost its second output
                            * 3: mcrt_render_rgba8, mcrt_render_rect */

/* error codes (0 = ok) */
#define MCRT_OK 0
#define MCRT_ERR_INVALID 1   /* bad argument / malformed scene description */
#define MCRT_ERR_NO_DEVICE 2 /* no HIP device, or HIP runtime failure */
#define MCRT_ERR_HIP 3       /* a HIP call failed; see mcrt_last_error() */
#define MCRT_ERR_NOMEM 4

/* ---- RayTracer::Config  (/root/reference/src/raytracer/raytracer.h:10-38) ---------------- */
typedef struct mcrt_config {
    int32_t width;             /* 256 */
    int32_t height;            /* 256 */
    int32_t max_bounces;       /* 3 */
    int32_t samples_per_pixel; /* 1 */
    int32_t tile_size;         /* 32; semantically significant: seeds the per-tile RNG */
    int32_t thread_count;      /* 0 = auto; accepted and ignored by the GPU path */
    int32_t soft_shadows;      /* bool, true */
    int32_t shadow_samples;    /* 8 */
    int32_t ao_enabled;        /* bool, false */
    int32_t ao_samples;        /* 8 */
    float ao_radius;           /* 3 */
    float ao_intensity;        /* .5 */
    int32_t dof_enabled;       /* bool, false */
    float aperture;            /* .5 */
    float focus_distance;      /* 0 = auto */
    int32_t gradient_bg;       /* bool, true */
    float gradient_scale;      /* 1 */
    float bg_center[4];        /* .91 .89 .86 1 */
    float bg_edge[4];          /* .56 .63 .71 1 */
} mcrt_config;

/* fills the struct with the in-class defaults of RayTracer::Config */
void mcrt_config_init(mcrt_config* cfg);

/* ---- Scene description: the reference's data model as POD -------------------------------
 * Scene/Light/Camera  /root/reference/src/scene/scene.h:10-34
 * Mesh                /root/reference/src/scene/mesh.h:12-27
 * Triangle            /root/reference/src/scene/triangle.h:9-16  (only v0..v2 and `texture`
 *                     are read by the ray tracer)
 * TextureRegion       /root/reference/src/skin/texture_region.h:8-27 */
typedef struct mcrt_texture {
    int32_t width;
    int32_t height;
    int64_t n_pixels;  /* pixels.size(); 0 ⇒ sample() returns Color() = (0,0,0,1) */
    const float* rgba; /* n_pixels * 4, row-major */
} mcrt_texture;

typedef struct mcrt_mesh {
    int32_t n_triangles;             /* mesh.triangles.size() (12 for a box) */
    const float* tri_vertices;       /* n_triangles * 9: v0.xyz v1.xyz v2.xyz */
    const int32_t* tri_texture;      /* n_triangles: index into scene textures, -1 = nullptr */
    int32_t n_local_triangles;       /* mesh.localTriangles.size() */
    const float* local_tri_vertices; /* n_local_triangles * 9 (unrotated box) */
    int32_t is_outer_layer;
    int32_t has_rotation;
    float pivot[3];
    float rot_x; /* degrees */
    float rot_z; /* degrees */
} mcrt_mesh;

typedef struct mcrt_scene_desc {
    int32_t n_meshes;
    const mcrt_mesh* meshes;
    int32_t n_textures;
    const mcrt_texture* textures;
    float light_position[3];
    float light_color[4];
    float light_intensity; /* unused by shade(), carried for completeness */
    float light_radius;
    float camera_position[3];
    float camera_target[3];
    float camera_up[3];
    float camera_fov; /* degrees */
    float background_color[4];
} mcrt_scene_desc;

/* ---- Tile  (/root/reference/src/raytracer/tile_renderer.h:11-14) -------------------------- */
typedef struct mcrt_tile {
    int32_t x, y, width, height;
} mcrt_tile;

/* TileRenderer::generateTiles (tile_renderer.cpp:18-39): row-major grid, edge tiles clipped,
 * zero tiles if any argument <= 0.  Returns the tile count; writes min(count, capacity) tiles
 * (tiles may be NULL to query the count). */
int mcrt_generate_tiles(int image_width, int image_height, int tile_size, mcrt_tile* tiles,
                        int capacity);

/* ---- library state ------------------------------------------------------------------------ */
int mcrt_abi_version(void);
/* number of HIP devices visible (0 when there is none; never fails) */
int mcrt_device_count(void);
/* message of the last failing call on this thread ("" if none) */
const char* mcrt_last_error(void);

/* ---- render: host buffers (the TileRenderer::render drop-in) ------------------------------
 * Renders the whole frame on `device` (>= 0; MCRT_DEVICE_ALL = every visible device, see
 * mcrt_render_multi) and copies it into out_rgba (width*height*4 floats, row-major, caller-owned).
 * Tile rows travel to the host as soon as they are final, while the rest of the frame still renders:
 * rows that hold only background right behind the first kernel, the rows of a pass behind that pass
 * when a large frame takes several.  `progress`, if non-NULL, is invoked exactly totalTiles times
 * with done = 1..total on the calling thread (tile_renderer.cpp:168-172 contract), for each row group
 * as it has landed in out_rgba.
 * Invalid sizes (any of width/height/tile_size <= 0) → MCRT_OK with nothing written, like the
 * reference returning an untouched Image (tile_renderer.cpp:144-146).  max_bounces above 4000 →
 * MCRT_ERR_INVALID (the workspace holds one colour per level and sample).
 * There is no CPU fallback: without a usable HIP device this returns MCRT_ERR_NO_DEVICE. */
typedef void (*mcrt_progress_fn)(int done, int total, void* user);
#define MCRT_DEVICE_ALL (-1)
int mcrt_render(const mcrt_scene_desc* scene, const mcrt_config* cfg, float* out_rgba,
                mcrt_progress_fn progress, void* user, int device);

/* The same frame spread over several devices of the node, one process: rank r of
 * n_devices renders tile rows r, r+n, r+2n, ... (cyclic — the figure occupies the middle rows) on
 * devices[r] with a replica of the scene; no collective inside the render.  devices = NULL or
 * n_devices <= 0: every visible device.  A device may be listed more than once (each entry is a rank
 * with its own workspace), which is how the path is tested on a one-GPU box.
 *   gather = 0  every device downloads its own rows straight into out_rgba: n PCIe links in parallel,
 *               no device-to-device traffic; the frame is assembled by the copies themselves
 *   gather = 1  the ranks' packed rows travel to devices[0] by peer copies (xGMI), one launch
 *               un-permutes them there (mcrt_assemble_frame_device), one download brings the frame back
 * Results are bit-identical to mcrt_render on one device.  Progress and errors as for mcrt_render. */
int mcrt_render_multi(const mcrt_scene_desc* scene, const mcrt_config* cfg, float* out_rgba,
                      mcrt_progress_fn progress, void* user, const int* devices, int n_devices, int gather);

/* The same render delivering the RGBA8 plane — `(uint8_t)(clamp(c,0,1)*255.0f+0.5f)` per channel, quantised in the
 * kernels' epilogue exactly like ImageWriter::writePNG / Image::toRGBA8 (image_writer.cpp:18-22, image.cpp:31-36) —
 * into out_rgba8 (width*height*4 bytes): 4 B per pixel on every link (PCIe, and xGMI when gather = 1) instead of 16.
 * devices / n_devices / gather as for mcrt_render_multi (one device: pass its index, n_devices = 1). */
int mcrt_render_rgba8(const mcrt_scene_desc* scene, const mcrt_config* cfg, uint8_t* out_rgba8, mcrt_progress_fn progress,
                      void* user, const int* devices, int n_devices, int gather);

/* TileRenderer::renderTile (tile_renderer.cpp:71-127): renders the one tile with row-major index
 * tile_index (generateTiles order) and writes its pixels into frame_rgba, a full width*height
 * float4 frame owned by the caller; all other pixels are left untouched. */
int mcrt_render_tile(const mcrt_scene_desc* scene, const mcrt_config* cfg, int tile_index,
                     float* frame_rgba, int device);
/* The same for an ARBITRARY Tile {x, y, width, height} of the frame, as the reference's renderTile accepts one: the
 * rectangle's own mt19937(tile.y * width + tile.x), its pixels in the rectangle's row-major order, cfg->tile_size not
 * read (tile_renderer.cpp:71-127).  An empty rectangle renders nothing; one that reaches outside the frame (the
 * reference would write out of bounds) → MCRT_ERR_INVALID.  A rectangle is one tile on the device — one RNG stream —
 * so a very large one renders correctly but far slower than mcrt_render of the same pixels. */
int mcrt_render_rect(const mcrt_scene_desc* scene, const mcrt_config* cfg, const mcrt_tile* tile, float* frame_rgba, int device);

/* ---- render: resident scene, device buffers (bench / multi-GPU path) --------------------- */
typedef struct mcrt_scene mcrt_scene; /* flattened scene resident in HBM on one device */

int mcrt_scene_create(const mcrt_scene_desc* desc, int device, mcrt_scene** out);
void mcrt_scene_destroy(mcrt_scene* scene);

/* out_layout */
#define MCRT_LAYOUT_FRAME 0  /* d_out is the full W*H float4 frame; only owned rows are written */
#define MCRT_LAYOUT_PACKED 1 /* d_out holds only the owned tile rows, packed in order */

/* Renders tile rows first, first+step, first+2*step, ... (a tile row = tile_size pixel rows) of
 * the frame into device memory on `stream` (a hipStream_t, NULL = default stream).  Asynchronous:
 * returns after enqueueing.  tile_row_first=0, tile_row_step=1 renders everything.
 * Sharding for N GPUs: rank r uses (first=r, step=N) — disjoint tile rows, no data-path
 * collective inside the render. */
int mcrt_render_device(mcrt_scene* scene, const mcrt_config* cfg, int tile_row_first,
                       int tile_row_step, int out_layout, float* d_out_rgba, void* stream);

/* mcrt_scene_destroy keeps the scene's device workspace (up to MCRT_POOL_MB, default 49152 MiB; one
 * idle set per device) for the next mcrt_scene_create / one-shot render on that device, because
 * allocating it dominates a single small render.  mcrt_trim() frees what is being kept. */
void mcrt_trim(void);
/* The library also keeps, per device that has rendered, a 128 MiB table of std::mt19937 seeding results
 * (state word 397 for the seeds -2^24 .. 2^24-1, which is where the per-hit shadow seeds of a scene at the
 * reference's scale lie): built once in ~2 ms, it replaces a 397-step recurrence per hit by one load, with
 * identical results.  MCRT_SEED_TABLE=0 turns it off; mcrt_trim() frees it when no scene handle is left. */
/* Sample table.  What a hit's soft-shadow samples are before the light enters — the cosine, the sine and the radius
 * factor of each light-disk sample — depends on the hit's shadow seed and the sample's index alone, not on the scene, the
 * light or the pose.  A device keeps them for the seeds -2^22 .. 2^22-1 (the built-in character's hits stay below 3.3 M
 * in magnitude) and up to 8 samples: 2^23 rows of 128 bytes, 1 GiB of the device's memory, filled in about a millisecond by
 * the routines the renderer itself runs, so frames are identical with and without it.  It is built at a device's SECOND
 * render with soft shadows of 2 .. 8 samples — a process that renders once never allocates it — and only where 3 GiB are
 * free; never inside a caller's stream capture (such a render does not read it either).  Seeds outside the window, more
 * than 8 samples, the extra-lights path and the stand-alone passes compute their samples as before.
 * MCRT_SAMPLE_TABLE=0 turns it off, =2 builds it at the first such render; mcrt_trim() frees it when no scene handle is left.
 * mcrt_sample_table_info: the bytes of the device's table (0: none) and how often it was built since the process began. */
int mcrt_sample_table_info(int device, size_t* bytes, int* builds);
/* The three per-device tables by one index: the window seed table (above, MCRT_SEED_TABLE), the table of all seeds (2^32
 * words, 16 GiB, built at a device's first ambient-occlusion render where three times that is free; MCRT_AO_SEED_TABLE=0 turns
 * it off) and the sample table. */
#define MCRT_TABLE_WINDOW 0
#define MCRT_TABLE_FULL 1
#define MCRT_TABLE_SAMPLE 2
/* the bytes of table `which` on `device` (0: none) and how often it was built there since the process began (either may be
 * NULL); which = MCRT_TABLE_SAMPLE gives what mcrt_sample_table_info gives.  MCRT_ERR_INVALID for another `which`. */
int mcrt_device_tables_info(int device, int which, size_t* bytes, int* builds);
/* *mask: bit `1 << which` is set where the handle holds table `which` right now, that is where its next render or pass reads
 * that table and not the recurrence or the engine (a render that the caller captures reads no sample table all the same). */
int mcrt_scene_tables(mcrt_scene* scene, int* mask);

/* Background plates.  The gradient background tiles of a frame (three quarters of the tiles of a 1080p frame of the
 * character) do not depend on the scene: their pixels are a function of width, height, tile_size, samples_per_pixel,
 * depth of field on / off, gradient_scale and the two gradient colours alone (the jitter comes from the tile's own
 * mt19937 stream).  The second time such a configuration is rendered on a device — every render call counts, a whole
 * frame, one rank's shard (a frame rendered as N shard calls is N renders) or a whole batch call alike; opaque gradient
 * background, 2 to 12 samples per pixel (6 under depth of field) — the library renders those tiles once
 * more into a plate kept on the device, tile by tile, and every later render of the configuration copies them from it:
 * identical pixels, a fifth fewer instructions per 1080p / 4 spp frame.  Building a plate costs about one render's first
 * kernel plus two allocations, synchronously inside that render call (never inside a caller's graph capture: such renders
 * take no plate).  Memory: ceil(width / tile_size) * ceil(height / tile_size) * tile_size^2 * 16 bytes per plate (1080p at
 * tile 32: 33.4 MB, 4K: 133.7 MB); at most 8 plates and MCRT_BG_PLATE_BUDGET_MB MiB per device — a configuration whose plate
 * does not fit gets none and renders as before — plates no scene handle uses make way for new ones, and mcrt_trim() frees
 * them.  A scene handle holds the plates of the four configurations it rendered last: a handle that goes through more
 * (a sweep of the gradient colour, say) waits, at each change to a configuration it does not hold, for its own previous
 * render — not for other handles' frames — and records its launch graphs for that plate anew; a render that builds a
 * plate, or frees one to make room, waits for the device as any allocation does.  A build that fails (memory refused) is
 * tried again 16 renders of the configuration later.  MCRT_BG_PLATE=0 turns plates off, MCRT_BG_PLATE=2 builds at a configuration's first render (development knobs). */
#define MCRT_BG_PLATE_BUDGET_MB 256
/* plates currently kept on `device`, their bytes, and how many were built there since the process began (any may be NULL) */
int mcrt_bg_plate_info(int device, int* plates, size_t* bytes, int* builds);

/* Draw plates.  The jitter and lens draws of a tile come from the tile's own mt19937 stream, seeded tile.y * width + tile.x:
 * they are a function of width, height, tile_size, samples_per_pixel and depth of field on / off alone — scene, pose, camera,
 * light, bounces and background do not enter.  The library keeps them like the background plates, under the same rules:
 * the second time such a configuration is rendered on a device (every render call counts; any background, the transparent
 * one included; up to 24 draws per pixel: 2 to 12 samples per pixel, 1 to 6 under depth of field; whole frames and shards,
 * not mcrt_render_rect) the draws of every tile of the frame are written once into a plate on the device, and later renders
 * read the draws of the tiles the figure touches from it instead of running each tile's chain of mt19937 twists again:
 * identical frames.  A configuration that takes both plates gets both in the same render call.  Memory:
 * ceil(width / tile_size) * ceil(height / tile_size) * tile_size^2 * samples_per_pixel * (2, or 4 under depth of field) * 4
 * bytes per plate (1080p at tile 32 and 4 spp: 66.8 MB, 4K: 267 MB); at most 4 plates and MCRT_DRAW_PLATE_BUDGET_MB MiB per
 * device.  Sightings, holding (four per scene handle and kind), eviction, failed builds, caller's graph captures and
 * mcrt_trim() are as for the background plates.  MCRT_DRAW_PLATE=0 turns draw plates off, MCRT_DRAW_PLATE=2 builds at a
 * configuration's first render (development knobs). */
#define MCRT_DRAW_PLATE_BUDGET_MB 512
/* draw plates currently kept on `device`, their bytes, and how many were built there since the process began (any may be NULL);
 * mcrt_bg_plate_info reports background plates only */
int mcrt_draw_plate_info(int device, int* plates, size_t* bytes, int* builds);

/* Work lists by ticket.  Within `primary` and `lit` a workgroup takes its first work item by its index and claims every later
 * one from an atomic counter of the pass, so that workgroups that drew cheap items take more of them (DESIGN.md §4 "Work
 * lists by ticket").  The frames do not depend on it.  MCRT_WORK_TICKETS=0 makes the workgroups stride over the lists by
 * the grid's size instead (development knob, read once per process like MCRT_BG_PLATE and MCRT_DRAW_PLATE). */

/* Waits for the scene's device work and reports an internal inconsistency of the last renders (the
 * workspace is sized for the tiles the host expects meshes to touch; the device flags a tile beyond
 * that bound instead of writing past it).  MCRT_OK in every correct run; the one-shot entry points
 * call it themselves. */
int mcrt_scene_check(mcrt_scene* scene);

/* A render is spread over internal *lanes* (streams with their own workspace, every n-th tile row of
 * the shard each, forked from / joined to the caller's stream) when the shard is large enough.
 * lanes = 0 restores that automatic choice, lanes >= 1 forces a count (at most 4).
 * One scene handle = one frame in flight: every render of a handle uses the handle's workspace, so
 * renders of one handle run one after the other on the device whatever streams they are given (the
 * library chains them with an event).  A caller that wants several frames in flight creates one
 * handle per frame in flight — and should then use lanes = 1, its frames already fill the chip.
 * Streams of the HIP runtime share its hardware queues (4 by default): more than 4 streams that
 * should run concurrently need GPU_MAX_HW_QUEUES set before the runtime initialises (bench.py: 8). */
int mcrt_scene_set_lanes(mcrt_scene* scene, int lanes);

/* Same render with the quantisation fused into the epilogue: writes the float4 frame to d_out_f32
 * and/or `(uint8_t)(clamp(c,0,1)*255.0f+0.5f)` per channel to d_out_rgba8 (either may be NULL, not
 * both) — the RGBA8 plane is what ImageWriter::writePNG hands to the PNG encoder
 * (/root/reference/src/output/image_writer.cpp:16-26), 4 B/pixel to copy back instead of 16. */
int mcrt_render_device_ex(mcrt_scene* scene, const mcrt_config* cfg, int tile_row_first, int tile_row_step,
                          int layout, float* d_out_f32, uint8_t* d_out_rgba8, void* stream);

/* ---- batches: many small frames in one launch sequence -------------------------------------------------------------
 * Frame i = exactly what mcrt_render_device_ex(scenes[i], cfg, 0, 1, MCRT_LAYOUT_FRAME, ...) would write, bit for bit.  All
 * frames share cfg and the device of scenes[0].  Frame i lives at d_out_f32 + i*frame_stride_pixels*4 floats and/or
 * d_out_rgba8 + i*frame_stride_pixels*4 bytes (either output may be NULL, not both; frame_stride_pixels >= width*height);
 * the pixels between frames are not written.  Asynchronous on `stream` (not into a graph being recorded on it).
 * Every frame that takes one pass on the flat pipeline goes through batched kernels, blockIdx.y = frame: one launch per
 * stage for up to 256 frames (larger batches take several launch sequences); any other frame (one that needs several
 * passes, or a config of the general variants such as max_bounces > 8) is enqueued on its own, one after the other.
 * Each handle's earlier renders are waited for and its next render waits for the batch, as for mcrt_render_device.
 * MCRT_ERR_INVALID, before any device work: n_frames < 0, a NULL entry, both outputs NULL, a stride below width*height,
 * a handle listed twice (each handle owns one workspace), handles on different devices, max_bounces above 4000.
 * Zero-size frames (width, height or tile_size <= 0) and n_frames = 0: MCRT_OK, nothing written. */
int mcrt_render_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, float* d_out_f32, uint8_t* d_out_rgba8,
                             size_t frame_stride_pixels, void* stream);
/* One-shot host form: n_frames scene descriptions -> n_frames*width*height*4 floats (out_rgba) and/or bytes (out_rgba8),
 * frame after frame, rendered on `device` with pooled handles, like mcrt_render. */
int mcrt_render_batch(const mcrt_scene_desc* const* scenes, int n_frames, const mcrt_config* cfg, float* out_rgba,
                      uint8_t* out_rgba8, int device);
/* How the last batch call on this thread ran: frames taken by the batched kernels, and launch sequences enqueued (1 when
 * the whole batch went through the batched kernels in one; each frame enqueued on its own counts one).  The frames of a
 * launch sequence share their background mode (mcrt_scene_set_background): a batch that mixes modes takes one sequence
 * per mode. */
int mcrt_last_batch_info(int* batched_frames, int* launch_sequences);

/* ---- background modes: the figure alone, on a transparent background -------------------------------------------------
 * MCRT_BACKGROUND_REFERENCE (the default everywhere): every pixel as the reference renders it (tile_renderer.cpp:89-124).
 * MCRT_BACKGROUND_TRANSPARENT: the same rays, the same mt19937 draws (jitter and lens draws are taken for samples that
 * miss too) and the same colour c_s for every sample s that hits — reflections still see the configured background, so
 * the figure looks exactly as in a reference render.  Of the S = max(1, spp) samples of a pixel, let A be the per-channel
 * float sum, in sample order, of c_s over the n samples whose primary ray hits (intersectScene(ray_s).hit, :111); the
 * samples that miss add nothing.  The pixel is (0, 0, 0, 0) when n = 0, else rgb = A.rgb * (1.0f / n) and
 * a = A.a * (1.0f / S), both reciprocals correctly rounded.  So a pixel whose samples all hit equals the reference pixel
 * bit for bit, a pixel without a hit is (0,0,0,0), and an edge pixel holds the mean colour of the figure's samples with
 * alpha = coverage x mean texel alpha: straight alpha, as PNG stores it (the RGBA8 plane is quantised as usual).
 * A `background` other than these two constants → MCRT_ERR_INVALID, checked right after the NULL-argument checks (before
 * the early return of a zero-size frame and before any device query).  Not available for mcrt_render_rect /
 * mcrt_render_tile. */
#define MCRT_BACKGROUND_REFERENCE 0
#define MCRT_BACKGROUND_TRANSPARENT 1
/* Per handle, like mcrt_scene_set_lanes: every later mcrt_render_device[_ex], mcrt_time_render_device and the handle's frame
 * in mcrt_render_batch_device use it.  A NULL handle → MCRT_ERR_INVALID. */
int mcrt_scene_set_background(mcrt_scene* scene, int background);
/* mcrt_render_multi (out_rgba) / mcrt_render_rgba8 (out_rgba8) with a background mode: exactly one of the two outputs
 * non-NULL, else MCRT_ERR_INVALID.  devices / n_devices / gather / progress as there. */
int mcrt_render_ex(const mcrt_scene_desc* scene, const mcrt_config* cfg, int background, float* out_rgba, uint8_t* out_rgba8,
                   mcrt_progress_fn progress, void* user, const int* devices, int n_devices, int gather);
/* mcrt_render_batch with a background mode for every frame */
int mcrt_render_batch_ex(const mcrt_scene_desc* const* scenes, int n_frames, const mcrt_config* cfg, int background, float* out_rgba,
                         uint8_t* out_rgba8, int device);
/* mcrt_render_png with a background mode (the transparent PNG: colour type 6, straight alpha) */
int mcrt_render_png_ex(const mcrt_scene_desc* scene, const mcrt_config* cfg, int background, const char* path, int device);

/* ---- extra lights: fill and rim lights in the beauty render ------------------------------------------------------------
 * The reference's Scene has one Light; a handle carries 0 to MCRT_MAX_EXTRA_LIGHTS more: light_1 .. light_K behind light_0,
 * the scene's own.  With K = 0 nothing changes anywhere.  With K >= 1 RayTracer::traceRay (raytracer.cpp:82-148) changes in
 * exactly one place — lines 107-117 become, in float32:
 *
 *     seed as today (one shadowSeed per hit and depth, shared by all lights)
 *     for k = 0 .. K:
 *         vis_k = config && softShadows && shadowSamples > 1
 *                   ? computeSoftShadow(hit.point, hit.normal, light_k, scene, shadowSamples, shadowSeed)
 *                   : -1
 *     C   = shade(hit, viewDir, light_0, scene, ShadingParams{}, vis_0)
 *     E_k = shade(hit, viewDir, light_k, scene, ShadingParams{kd, ks, ambient = 0, shininess}, vis_k)      k = 1 .. K
 *     shadedColor.rgb = clamp(((C.rgb + E_1.rgb) + E_2.rgb) + E_3.rgb, 0, 1);   shadedColor.a = C.a
 *
 * computeSoftShadow (shading.cpp:28-60) decides by light_k's OWN radius between the disk and the single ray (:30), and every
 * light draws the SAME 2 * shadowSamples mt19937 draws of the hit: one seeding chain per hit, K + 1 disks.  vis_k = -1 is
 * shade()'s own isInShadow test with the normalised normal (:76-81).  C and every E_k are clamped by shade() itself (:95),
 * the sum runs left to right.  Ambient occlusion at depth 0, the reflection fold (:133-147), renderTile's sample loop and
 * the background are untouched.  A light whose colour is (0, 0, 0) adds exactly +0: the frame is then the single-light frame
 * bit for bit.
 * The beauty renders of a handle honour its extra lights: mcrt_render_device[_ex], mcrt_time_render_device, the handle's
 * frame in mcrt_render_batch_device (it is then enqueued on its own), row shards and both background modes.  The lights
 * survive mcrt_scene_set_skin* and mcrt_scene_set_view*.  The passes whose result depends on the light — ground shadow,
 * reflection, light layers, light bake and every studio-shot entry — return MCRT_ERR_INVALID ("extra lights: beauty render
 * only") for a handle with K >= 1, and work again after n = 0; layers, picks and ground occlusion run unchanged.
 * mcrt_probe_trace ignores extra lights. */
#define MCRT_MAX_EXTRA_LIGHTS 3
typedef struct mcrt_light_source {
    float position[3];
    float radius;   /* < 1e-4: a point light */
    float color[4]; /* rgb; the fourth channel is not read */
} mcrt_light_source; /* 32 bytes */
/* n = 0: none, the handle is as before.  A NULL handle, n < 0 or n > MCRT_MAX_EXTRA_LIGHTS, lights NULL with n > 0, a
 * position, radius or colour component that is not finite → MCRT_ERR_INVALID, before any device work.  Host state only:
 * renders enqueued before the call keep the lights they were enqueued with. */
int mcrt_scene_set_extra_lights(mcrt_scene* scene, const mcrt_light_source* lights, int n);
/* Returns the handle's count and copies min(count, capacity) lights into out (which may be NULL); a NULL handle: 0. */
int mcrt_scene_extra_lights(const mcrt_scene* scene, mcrt_light_source* out, int capacity);
/* mcrt_render_ex with extra lights (n_lights = 0: mcrt_render_ex itself); the same argument checks as
 * mcrt_scene_set_extra_lights, right behind the NULL-argument checks. */
int mcrt_render_lights(const mcrt_scene_desc* scene, const mcrt_config* cfg, const mcrt_light_source* lights, int n_lights, int background,
                       float* out_rgba, uint8_t* out_rgba8, mcrt_progress_fn progress, void* user, const int* devices, int n_devices, int gather);
/* mcrt_render_png_ex with extra lights */
int mcrt_render_png_lights(const mcrt_scene_desc* scene, const mcrt_config* cfg, const mcrt_light_source* lights, int n_lights, int background,
                           const char* path, int device);

/* ---- geometry layers: what is under each pixel ----------------------------------------------------------------------
 * One ray per pixel through the pixel centre — u = (px + 0.5f) / width, v = (py + 0.5f) / height, Camera::generateRay(u, v,
 * (float)width / (float)height): the reference's own primary ray at samplesPerPixel == 1 without depth of field
 * (tile_renderer.cpp:92-103) — and the surface intersectScene finds for it (intersection.cpp:408-421).  No draws, no shading:
 * of mcrt_config only width, height and tile_size are read (tile_size is the granularity of the culling and never changes a
 * value); samples_per_pixel, depth of field, max_bounces, the shadow and ambient-occlusion settings and the background fields
 * are IGNORED, and so is the handle's background mode.  Each layer is a plane of width * height pixels, row-major:
 *   depth   1 float   HitResult::t                                   miss: FLT_MAX (what intersectScene leaves in t)
 *   normal  4 floats  HitResult::normal, w = 0                       miss: 0 0 0 0
 *   albedo  4 floats  HitResult::textureColor                        miss: 0 0 0 0
 *   id      4 int32   {mesh, face, tx, ty}                           miss: {-1, 0, -1, -1}
 * mesh: index into scene.meshes (the first mesh on a tie in t, as in the reference).  face & 7: the face slot in determineFace
 * order — 0 back (-Z), 1 front (+Z), 2 left (+X), 3 right (-X), 4 top, 5 bottom; face & MCRT_ID_BACK: the hit is the outer
 * layer's exit face (intersection.cpp:349-357); face & MCRT_ID_OUTER: HitResult::isOuterLayer.  tx, ty: the texel of the face's
 * TextureRegion that sample() read; -1, -1 for a face without a texture or with an empty one (albedo then holds the reference's
 * magenta or Color()).  Depth, normal and albedo are bit-identical to the reference's HitResult; a pixel whose id.mesh is -1 is
 * (0,0,0,0) in the MCRT_BACKGROUND_TRANSPARENT frame of the same scene at samples_per_pixel 1 without depth of field.
 * A layers pass reads the scene alone: it uses none of the handle's workspace, so it may run beside the handle's render on
 * another stream; mcrt_scene_destroy and mcrt_scene_check wait for it.  Whole frames only (no tile-row shards, no packed
 * layout, no lanes, not into a graph being recorded).
 * MCRT_ERR_INVALID before any device work: a NULL config, handle, entry or layers struct, all four planes NULL, n < 0, a stride
 * below width * height, handles on different devices.  Zero-size frames (width, height or tile_size <= 0) and n_frames = 0:
 * MCRT_OK, nothing written. */
#define MCRT_ID_BACK 8
#define MCRT_ID_OUTER 16
typedef struct mcrt_layers {
    float* depth;  /* any may be NULL (that plane is not produced), not all */
    float* normal;
    float* albedo;
    int32_t* id;
} mcrt_layers;
/* resident scene, device pointers, asynchronous on `stream` */
int mcrt_render_layers_device(mcrt_scene* scene, const mcrt_config* cfg, const mcrt_layers* d_out, void* stream);
/* n_frames scenes of one config in one launch, frame i at each plane + i * frame_stride_pixels pixels (>= width * height; the
 * pixels between frames are not written).  A handle may be listed more than once. */
int mcrt_render_layers_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_layers* d_out,
                                    size_t frame_stride_pixels, void* stream);
/* one-shot host forms: host pointers, rendered on `device` with pooled handles like mcrt_render; frame after frame */
int mcrt_render_layers(const mcrt_scene_desc* scene, const mcrt_config* cfg, const mcrt_layers* out, int device);
int mcrt_render_layers_batch(const mcrt_scene_desc* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_layers* out, int device);

/* Picking: the same question for n pixels, xy = n x {x, y} (host memory), one record per pixel into out (host memory): the
 * four id fields, then depth, HitResult::point (0 0 0 at a miss), normal and albedo as in the planes — equal to the planes at
 * that pixel.  Synchronous: one small launch, one small download.  A coordinate outside the frame → MCRT_ERR_INVALID (n = 0:
 * MCRT_OK). */
typedef struct mcrt_surface {
    int32_t mesh, face, tx, ty;
    float t;
    float point[3];
    float normal[4];
    float albedo[4];
} mcrt_surface; /* 64 bytes */
int mcrt_scene_pick(mcrt_scene* scene, const mcrt_config* cfg, const int32_t* xy, int n, mcrt_surface* out);

/* Skin coordinates (host only): (mesh, face slot 0..5, tx, ty) of a scene built by mcrt_build_skin_scene → the texel (x, y) of
 * the skin image that face texel was cut from, by the builder's own tables (the mirrored left limbs of a legacy 64x32 skin
 * included) — what an editor paints when the user clicks a pixel.  skin_height 64: meshes 0..11 = {head, body, right arm, left
 * arm, right leg, left leg} x {inner, outer}; 32: 0 head, 1 head's outer layer, 2 body, 3 right arm, 4 left arm, 5 right leg,
 * 6 left leg.  (The builder drops an outer part whose texels are all transparent, which moves the later meshes up: such a scene
 * has fewer meshes than these tables.)  MCRT_ERR_INVALID for an argument out of range for that skin kind. */
int mcrt_skin_texel(int skin_height, int mesh, int face_slot, int tx, int ty, int* skin_x, int* skin_y);

/* ---- ground shadow: the figure's soft shadow on a floor plane, as a layer of its own --------------------------------------
 * The reference's scene has no floor; this pass answers, per pixel, how much of the light reaches the point of the plane
 * y = ground_y under that pixel — what a compositor puts under the MCRT_BACKGROUND_TRANSPARENT figure.  The ray is the geometry
 * layers': u = (px + 0.5f) / width, v = (py + 0.5f) / height, Camera::generateRay(u, v, (float)width / (float)height), origin o
 * and direction d.  The plane's normal is N = (0, 1, 0) from either side.  All arithmetic float32, uncontracted:
 *   t = (ground_y - o.y) / d.y                      the pixel REACHES the plane iff d.y != 0 && t > 0 && t <= FLT_MAX
 *   P = (o.x + d.x * t, ground_y, o.z + d.z * t)
 *   seed = (unsigned)(P.x * 12345.0f + P.y * 67890.0f + P.z * 11111.0f)      summed left to right, the reference's cast
 *                                                   (raytracer.cpp:110-112 at depth 0)
 *   S = shadow_samples when soft_shadows && shadow_samples > 1, else 1
 *   visibility = computeSoftShadow(P, N, scene.light, scene, S, seed)        (shading.cpp:28-60; at S = 1 or with a light
 *                                                   radius below 1e-4 the one isInShadow ray)
 * The figure in front of the plane plays no part: the shadow is computed for every pixel that reaches the plane (an edge pixel
 * of the transparent figure shows the ground through it).  Planes of width * height pixels, row-major:
 *   visibility  1 float   the value above (k / S)                                  not reached: 1.0f
 *   distance    1 float   t                                                        not reached: FLT_MAX
 *   matte       1 uint8   (uint8_t)(clamp(1.0f - visibility, 0, 1) * 255.0f + 0.5f)   not reached: 0
 * matte is the alpha of a black shadow image, quantised as mcrt_quantize_rgba8 quantises a channel: page * (1 - matte / 255)
 * under the straight-alpha figure.  Of mcrt_config the pass reads width, height, tile_size (the granularity of the culling,
 * never a value), soft_shadows and shadow_samples; everything else and the handle's background mode are IGNORED.  The values
 * are bit-identical to the reference's computeSoftShadow at those points.
 * shadow_samples is limited to 113 when soft_shadows is on (MCRT_ERR_INVALID above): the pass draws a pixel's light samples
 * from the truncated mt19937 form, which yields the first 227 draws of an engine and keeps no 624-word state per lane.
 * The rules of the geometry layers hold: whole frames only; asynchronous on `stream`, not into a graph being recorded; no
 * workspace, no counters and none of the handle's events, so the pass may run beside the handle's render on another stream;
 * mcrt_scene_destroy and mcrt_scene_check wait for it; a handle may be listed more than once in a batch, with different
 * ground_y; the pixels between frames are not written.
 * MCRT_ERR_INVALID before any device work: a NULL config, handle, entry, ground_y array or planes struct, all three planes
 * NULL, n_frames < 0, a stride below width * height, handles on different devices, a ground_y that is not finite,
 * soft_shadows && shadow_samples > 113.  Zero-size frames and n_frames = 0: MCRT_OK, nothing written. */
typedef struct mcrt_ground {
    float* visibility; /* any may be NULL (that plane is not produced), not all */
    float* distance;
    uint8_t* matte;
} mcrt_ground;
/* resident scene, device pointers, asynchronous on `stream` */
int mcrt_render_ground_device(mcrt_scene* scene, const mcrt_config* cfg, float ground_y, const mcrt_ground* d_out, void* stream);
/* n_frames scenes of one config in one launch; ground_y: n_frames heights in HOST memory (read before the call returns); frame i
 * at each plane + i * frame_stride_pixels pixels */
int mcrt_render_ground_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const float* ground_y,
                                    const mcrt_ground* d_out, size_t frame_stride_pixels, void* stream);
/* one-shot host form: host pointers, rendered on `device` with a pooled handle like mcrt_render */
int mcrt_render_ground(const mcrt_scene_desc* scene, const mcrt_config* cfg, float ground_y, const mcrt_ground* out, int device);
/* The floor of a scene (host only): the smallest y of all tri_vertices — the posed, world-space boxes, so a lifted leg counts.
 * At pose 0 that is 0.0 for the built-in default scene and for a 64x32 skin, and -0.5 for a 64x64 skin: its outer leg layers
 * are boxes 0.5 larger than the legs on every side, and they are vertices like any other.  A plane at that floor lies 0.5
 * below the soles of such a figure, so the shadow does not touch the feet; pass the height of the soles (0.0 for the builder's
 * standing poses) for a contact shadow.  A scene without a vertex (or a NULL argument) → MCRT_ERR_INVALID. */
int mcrt_scene_floor(const mcrt_scene_desc* scene, float* y);

/* ---- ground occlusion: the figure's contact occlusion on a floor plane, as a layer of its own -----------------------------
 * The ground shadow is the disk light's shadow alone: it falls away from the light, so the floor between and right around the
 * feet stays fully lit.  This pass answers, per pixel, how open the hemisphere above the point of the plane y = ground_y under
 * that pixel is — the reference's ambient occlusion, asked at the floor.  The ray, the plane hit, t and P are the ground
 * shadow's: the pixel-centre ray, t = (ground_y - o.y) / d.y, the pixel REACHES the plane iff d.y != 0 && t > 0 && t <= FLT_MAX,
 * P = (o.x + d.x * t, ground_y, o.z + d.z * t), N = (0, 1, 0) from either side.  All arithmetic float32, uncontracted:
 *   seed      = (unsigned)(P.x * 73856093.0f + P.y * 19349663.0f + P.z * 83492791.0f)     summed left to right, the reference's
 *                                                   cast (raytracer.cpp:122-123)
 *   occlusion = computeAO(P, N, scene, ao_samples, ao_radius, seed)                        (raytracer.cpp:38-78)
 *             = 1 - occluded / ao_samples           occluded: the samples whose ray from P + N * 1e-3f meets a mesh before ao_radius
 * The figure in front of the plane plays no part.  Planes of width * height pixels, row-major:
 *   occlusion   1 float   the value above                                               not reached: 1.0f
 *   matte       1 uint8   (uint8_t)(clamp(1.0f - occlusion, 0, 1) * 255.0f + 0.5f)         not reached: 0
 * The distance plane is the ground pass's and is not repeated.  Of mcrt_config the pass reads width, height, tile_size (the
 * granularity of the culling, never a value), ao_samples and ao_radius; everything else — ao_enabled, ao_intensity, the shadow
 * fields — and the handle's background mode are IGNORED.  The values are bit-identical to the reference's computeAO at those
 * points.  ao_radius <= 0 is legal: no ray can be occluded, every value is 1.0f and nothing is traced.
 * ao_samples is limited to 1 .. 113 (MCRT_ERR_INVALID outside): the reference divides by it, and the pass draws a pixel's
 * samples from the truncated mt19937 form, which yields the first 227 draws of an engine — a sample takes two.
 * The rules of the ground shadow hold word for word: whole frames only; asynchronous on `stream`, not into a graph being
 * recorded; no workspace, no counters and none of the handle's events, so the pass may run beside the handle's render on
 * another stream; it reads the device's seed tables through the handle and builds none; mcrt_scene_destroy and
 * mcrt_scene_check wait for it; a handle may be listed more than once in a batch, with different ground_y; the pixels between
 * frames are not written; ground_y of a batch is host memory read before the call returns.
 * MCRT_ERR_INVALID before any device work: a NULL config, handle, entry, ground_y array or planes struct, both planes NULL,
 * n_frames < 0, a stride below width * height, handles on different devices, a ground_y that is not finite, ao_samples < 1,
 * ao_samples > 113, an ao_radius that is not finite.  Zero-size frames and n_frames = 0: MCRT_OK, nothing written. */
typedef struct mcrt_ground_occlusion {
    float* occlusion; /* either may be NULL (that plane is not produced), not both */
    uint8_t* matte;
} mcrt_ground_occlusion;
/* resident scene, device pointers, asynchronous on `stream` */
int mcrt_render_ground_occlusion_device(mcrt_scene* scene, const mcrt_config* cfg, float ground_y, const mcrt_ground_occlusion* d_out,
                                        void* stream);
/* n_frames scenes of one config in one launch; ground_y: n_frames heights in HOST memory (read before the call returns); frame i
 * at each plane + i * frame_stride_pixels pixels */
int mcrt_render_ground_occlusion_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const float* ground_y,
                                              const mcrt_ground_occlusion* d_out, size_t frame_stride_pixels, void* stream);
/* one-shot host form: host pointers, rendered on `device` with a pooled handle like mcrt_render */
int mcrt_render_ground_occlusion(const mcrt_scene_desc* scene, const mcrt_config* cfg, float ground_y, const mcrt_ground_occlusion* out,
                                 int device);

/* ---- ground reflection: the figure mirrored in a floor plane, as a layer of its own ---------------------------------------
 * The other half of a figure standing on a glossy floor: per pixel, the colour the reference's own recursion would return for
 * the reflection ray of a floor at y = ground_y — traceRay(reflectRay, depth + 1) (raytracer.cpp:133-142) with the floor as the
 * depth-0 surface.  A flipped copy of the figure cannot replace it: it shows the wrong faces and does not meet the feet.
 * The ray is the geometry layers' pixel-centre ray, origin o and direction d; the plane point is the ground shadow's, with
 * N = (0, 1, 0) from either side.  All arithmetic float32 with one rounding per operation, uncontracted:
 *   t = (ground_y - o.y) / d.y                      the pixel REACHES the plane iff d.y != 0 && t > 0 && t <= FLT_MAX
 *   P = (o.x + d.x * t, ground_y, o.z + d.z * t)
 *   reflection ray = the reference's own (raytracer.cpp:134-140) for a hit at P with normal N and incoming direction d:
 *     Nn = normalize(N); D = normalize(d); R = normalize(D - Nn * (2 * dot(D, Nn))); origin = P + Nn * 1e-3f
 *   hit = intersectScene(reflection ray)
 *   colour = traceRay(reflection ray, depth = 1, maxBounces = cfg.max_bounces)      where hit.hit
 * So the shadow seed of the reflected hit carries + 1 * 99999.0f, no ambient occlusion applies (the reference computes it at
 * depth 0 only), the chain may bounce on to max_bounces, and a bounced miss folds scene.backgroundColor, flat.  Alpha is the hit
 * texel's originalAlpha.  Planes of width * height pixels, row-major:
 *   rgba      4 floats  the colour above, straight alpha                                    no reflected hit: (0, 0, 0, 0)
 *   rgba8     4 uint8   each channel (uint8_t)(clamp(c, 0, 1) * 255.0f + 0.5f), as mcrt_quantize_rgba8    no hit: 0, 0, 0, 0
 *   distance  1 float   HitResult::t of the reflection ray's closest hit                   no reflected hit: FLT_MAX
 * ("no reflected hit": the pixel does not reach the plane, or its reflection ray misses the scene.)
 * With the ground shadow's matte m, this layer R and a floor reflectivity k of the compositor's choice (possibly faded by
 * distance), the floor under the straight-alpha figure is   page * (1 - m) * (1 - k * R.a) + R.rgb * k * R.a.
 * Of mcrt_config the pass reads width, height, tile_size (the granularity of the culling, never a value), max_bounces,
 * soft_shadows and shadow_samples; everything else — the ambient-occlusion fields, depth of field, samples_per_pixel, the
 * gradient — and the handle's background mode are IGNORED.  max_bounces < 1: the reference returns before it intersects
 * (depth > maxBounces); the call returns MCRT_OK and every pixel gets the no-hit constants.
 * The rules of the ground shadow hold: whole frames only; asynchronous on `stream`, not into a graph being recorded; no
 * workspace, no counters and none of the handle's events; the pass reads the device's seed table through the handle;
 * mcrt_scene_destroy and mcrt_scene_check wait for it; a handle may be listed more than once in a batch, with different
 * ground_y; the pixels between frames are not written.
 * MCRT_ERR_INVALID before any device work: everything the ground shadow refuses (a NULL config, handle, entry, ground_y array
 * or planes struct, n_frames < 0, a stride below width * height, handles on different devices), all three planes NULL, a
 * ground_y that is not finite, soft_shadows && shadow_samples > 113 (as for the ground shadow), max_bounces > 8 (the chain's
 * level colours are folded back to front from a stack of that depth, the depth the render pipeline's arrays are laid out for).
 * Zero-size frames and n_frames = 0: MCRT_OK, nothing written.
 * MCRT_REFLECT_CULL=0 in the environment turns the pass's tile culling off (a development knob: the values do not change). */
typedef struct mcrt_reflection {
    float* rgba; /* any may be NULL (that plane is not produced), not all */
    uint8_t* rgba8;
    float* distance;
} mcrt_reflection;
/* resident scene, device pointers, asynchronous on `stream` */
int mcrt_render_reflection_device(mcrt_scene* scene, const mcrt_config* cfg, float ground_y, const mcrt_reflection* d_out, void* stream);
/* n_frames scenes of one config in one launch; ground_y: n_frames heights in HOST memory (read before the call returns); frame i
 * at each plane + i * frame_stride_pixels pixels */
int mcrt_render_reflection_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const float* ground_y,
                                        const mcrt_reflection* d_out, size_t frame_stride_pixels, void* stream);
/* one-shot host form: host pointers, rendered on `device` with a pooled handle like mcrt_render */
int mcrt_render_reflection(const mcrt_scene_desc* scene, const mcrt_config* cfg, float ground_y, const mcrt_reflection* out, int device);

/* ---- light layers: per-pixel shadow, ambient occlusion and direct light on the figure itself ------------------------------
 * The terms a relighting or an "ambient occlusion only" look is built from: how much of the disk light reaches the surface under
 * a pixel, how occluded that surface is, and what shade() returns for it before ambient occlusion and the bounces are folded in
 * — the reference's own computeSoftShadow, computeAO and shade at the primary hit.
 * The ray is the geometry layers' ray: u = (px + 0.5f) / width, v = (py + 0.5f) / height, Camera::generateRay(u, v,
 * (float)width / (float)height) with origin o, and h = intersectScene(ray).  All arithmetic float32 with one rounding per
 * operation, uncontracted.  For a pixel with h.hit (planes of width * height pixels, row-major):
 *   visibility  1 float   the value shade() multiplies diffuse and specular by in traceRay at depth 0 (raytracer.cpp:107-117,
 *                         shading.cpp:76-81), in one of three modes:
 *                           soft_shadows && shadow_samples > 1:
 *                             computeSoftShadow(h.point, h.normal, scene.light, scene, shadow_samples, seed) with
 *                             seed = (unsigned)(p.x * 12345.0f + p.y * 67890.0f + p.z * 11111.0f + 0.0f * 99999.0f), summed left
 *                             to right, the reference's cast; inside it a light radius below 1e-4 takes the one isInShadow ray
 *                             with the raw normal;
 *                           otherwise shade()'s own fallback: isInShadow(h.point, normalize(h.normal), light.position) ? 0 : 1
 *   occlusion   1 float   computeAO(h.point, h.normal, scene, ao_samples, ao_radius, aoSeed) = 1 - occluded / ao_samples with
 *                         aoSeed = (unsigned)(p.x * 73856093.0f + p.y * 19349663.0f + p.z * 83492791.0f) (raytracer.cpp:38-78,
 *                         :122-123).  Produced whenever the plane is asked for: ao_enabled and ao_intensity are IGNORED, the
 *                         compositor applies 1 - k * (1 - occlusion) itself
 *   direct      4 floats  shade(h, normalize(o - h.point), scene.light, scene, ShadingParams{}, visibility): shadedColor of
 *                         raytracer.cpp:117 — Blinn-Phong, clamped, alpha = the texel's alpha
 * At a miss: visibility 1.0f, occlusion 1.0f, direct (0, 0, 0, 0).
 * RECOMPOSITION (part of the contract).  For every pixel with a hit, the beauty frame of the same scene at samples_per_pixel = 1,
 * no depth of field, max_bounces = 0 and the same shadow settings
 *   - with ao_enabled = 0 EQUALS direct, bit for bit;
 *   - with ao_enabled = 1 equals, for that config's ao_samples, ao_radius and ao_intensity,
 *       k = 1.0f - ao_intensity * (1.0f - occlusion);  rgb = clamp(direct.rgb * k, 0, 1);  a = direct.a
 *     bit for bit.
 * Of mcrt_config the pass reads width, height, tile_size (the granularity of the culling, never a value), soft_shadows,
 * shadow_samples, ao_samples and ao_radius (the last two only when the occlusion plane is asked for); everything else and the
 * handle's background mode are IGNORED.  ao_radius <= 0 is legal: no ray can be occluded, the plane is 1.0f.
 * The rules of the geometry layers hold: whole frames only; asynchronous on `stream`, not into a graph being recorded; no
 * workspace, no counters and none of the handle's events, so the pass may run beside the handle's render on another stream; the
 * pass reads the device's seed tables through the handle and builds none; mcrt_scene_destroy and mcrt_scene_check wait for it;
 * a handle may be listed more than once in a batch; the pixels between frames are not written.
 * MCRT_ERR_INVALID before any device work: everything the ground shadow refuses (a NULL config, handle, entry or planes struct,
 * all three planes NULL, n_frames < 0, a stride below width * height, handles on different devices), soft_shadows &&
 * shadow_samples > 113 (the truncated mt19937 form yields 227 draws), and, when the occlusion plane is asked for, ao_samples < 1
 * (the reference divides by it), ao_samples > 113 (an AO sample takes two draws) or an ao_radius that is not finite.
 * Zero-size frames and n_frames = 0: MCRT_OK, nothing written. */
typedef struct mcrt_light_planes {
    float* visibility; /* any may be NULL (that plane is not produced), not all */
    float* occlusion;
    float* direct;
} mcrt_light_planes;
/* resident scene, device pointers, asynchronous on `stream` */
int mcrt_render_light_device(mcrt_scene* scene, const mcrt_config* cfg, const mcrt_light_planes* d_out, void* stream);
/* n_frames scenes of one config in one launch per kernel; frame i at each plane + i * frame_stride_pixels pixels */
int mcrt_render_light_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_light_planes* d_out,
                                   size_t frame_stride_pixels, void* stream);
/* one-shot host form: host pointers, rendered on `device` with a pooled handle like mcrt_render */
int mcrt_render_light(const mcrt_scene_desc* scene, const mcrt_config* cfg, const mcrt_light_planes* out, int device);

/* ---- light bake: per-texel shadow, ambient occlusion and direct light in texture space ------------------------------------
 * The terms of the light layers on the skin itself instead of on a view of it: for every texel of every face how much of the
 * disk light reaches it, how occluded it is and what shade() makes of it — a light map, an ambient-occlusion bake, a pre-shaded
 * skin.  No camera enters: the faces where the arm meets the body are baked like any other.  All arithmetic float32 with one
 * rounding per operation, uncontracted, in the order written; every division is correctly rounded.
 * OWNER FACE.  Face slot f (0..5, determineFace order: 0 back -Z, 1 front +Z, 2 left +X, 3 right -X, 4 top, 5 bottom) of mesh m
 * with a texture references the pool texels tex_off[f] ... tex_off[f] + w * h - 1, row-major.  Faces may share a texture, so a
 * pool texel is baked on its OWNER: of the faces that reference it the one with the lowest mesh index, then the lowest face
 * slot.  A texel no face references has no owner.  mcrt_bake_texel_table (host only, no device) returns the number of pool
 * texels n_texels, or -1 with MCRT_ERR_INVALID's text for a scene that cannot be flattened, and writes for the first
 * min(n_texels, capacity) texels {mesh, face, tx, ty}, {-1, 0, -1, -1} without an owner.  The planes are indexed like this
 * table.  For a repaintable handle it agrees with mcrt_skin_pool_map / mcrt_skin_texel.
 * SAMPLE POINTS.  grid = q, 1..4.  Sub-sample (i, j), 0 <= i, j < q, of texel (tx, ty) of a w x h face:
 *     u = ((float)tx + ((float)i + 0.5f) / (float)q) / (float)w        v = ((float)ty + ((float)j + 0.5f) / (float)q) / (float)h
 * The local point p is the inverse of computeFaceUV (intersection.cpp:136-196) on the face's plane, with lo, hi the mesh's
 * box, ext = hi - lo and neg = the face on the min side of its axis (slots 0, 3, 5):
 *     slots 0, 1 (axis z)   lx = neg ? 1.0f - u : u,  ly = 1.0f - v   p = (lo.x + lx * ext.x, lo.y + ly * ext.y, neg ? lo.z : hi.z)
 *     slots 2, 3 (axis x)   lz = neg ? u : 1.0f - u,  ly = 1.0f - v   p = (neg ? lo.x : hi.x, lo.y + ly * ext.y, lo.z + lz * ext.z)
 *     slots 4, 5 (axis y)   lx = u,  lz = neg ? 1.0f - v : v          p = (lo.x + lx * ext.x, neg ? lo.y : hi.y, lo.z + lz * ext.z)
 * P = rotatePoint(p) forwards (rotX, then rotZ, about the pivot: the reference's hit point, intersection.cpp:399) for a mesh with
 * hasRotation, p otherwise.  N is the normal intersectMesh gives a front hit of that face: the face's axis vector, and for a
 * mesh with hasRotation normalize(rotateDir(n)) (intersection.cpp:400).
 * PER SUB-SAMPLE, the light layers' terms with P, N in place of the hit:
 *   vis   soft_shadows && shadow_samples > 1: computeSoftShadow(P, N, light, scene, shadow_samples, seed) with
 *         seed = (unsigned)(P.x * 12345.0f + P.y * 67890.0f + P.z * 11111.0f + 0.0f * 99999.0f); otherwise
 *         isInShadow(P, normalize(N), light.position) ? 0 : 1
 *   occ   computeAO(P, N, scene, ao_samples, ao_radius, (unsigned)(P.x * 73856093.0f + P.y * 19349663.0f + P.z * 83492791.0f)),
 *         whatever ao_enabled says
 *   dir   shade(hit{P, N, the texel's colour, isOuterLayer of the mesh}, viewDir = N, light, scene, ShadingParams{}, vis); its
 *         alpha is the texel's.  A texel has no camera: the view vector is the normal, the usual convention of a bake.
 * PLANES, in pool order.  A texel is DEAD when it has no owner or its alpha == 0.0f, LIVE otherwise.  "Mean": the q * q
 * sub-sample values added left to right, j outer and i inner, starting from the first value, then divided by (float)(q * q);
 * with q = 1 the value itself.
 *   position    4 floats  P of the texel centre (the q = 1 formula), w = 1.0f; dead: the same point with w = 0.0f, all zero
 *                         without an owner
 *   normal      4 floats  N, w = 0.0f; zero without an owner
 *   visibility  1 float   mean of vis; dead: 1.0f
 *   occlusion   1 float   mean of occ; dead: 1.0f
 *   direct      4 floats  componentwise mean of dir; dead: (0, 0, 0, 0)
 * Of mcrt_config the pass reads soft_shadows, shadow_samples, ao_samples and ao_radius (the last two only when the occlusion
 * plane is asked for) and nothing else — no frame size —, and not the handle's background mode.
 * Asynchronous on `stream`, not into a graph being recorded (a batch); no workspace, no counters and none of the handle's
 * events, so a bake may run beside the handle's render on another stream; it reads the device's seed tables through the handle
 * and builds none; mcrt_scene_destroy and mcrt_scene_check wait for it.  Ordering a bake against a REPAINT of the handle
 * (mcrt_scene_set_skin_device & co) — stream order, or an event of the caller's — is the caller's job, as for the layers.
 * Batch: frame i starts i * texel_stride texels on in every plane; the scenes may hold different numbers of texels, and
 * texel_stride is at least the largest; the texels between frames are not written; a handle may be listed more than once; one
 * launch per kernel and 4096 frames.
 * MCRT_ERR_INVALID before any device work, the planes untouched: a NULL config, handle, entry or planes struct; all five
 * planes NULL; n_frames < 0; handles on different devices; grid outside 1..4; a texel_stride below a scene's texel count;
 * soft_shadows && shadow_samples > 113; and, when the occlusion plane is asked for, ao_samples < 1, ao_samples > 113 or an
 * ao_radius that is not finite.  n_frames = 0 and scenes without texels: MCRT_OK, nothing written. */
typedef struct mcrt_bake_planes {
    float* position; /* any may be NULL (that plane is not produced), not all */
    float* normal;
    float* visibility;
    float* occlusion;
    float* direct;
} mcrt_bake_planes;
/* resident scene, device pointers, asynchronous on `stream` */
int mcrt_bake_light_device(mcrt_scene* scene, const mcrt_config* cfg, int grid, const mcrt_bake_planes* d_out, void* stream);
int mcrt_bake_light_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, int grid, const mcrt_bake_planes* d_out,
                                 size_t texel_stride, void* stream);
/* one-shot host form: host pointers (mcrt_bake_texel_table's count of texels per plane), baked on `device` with a pooled handle */
int mcrt_bake_light(const mcrt_scene_desc* scene, const mcrt_config* cfg, int grid, const mcrt_bake_planes* out, int device);
int mcrt_bake_texel_table(const mcrt_scene_desc* scene, int32_t (*out)[4], int capacity);
/* the number of pool texels of a resident scene: the texels per plane of its bake */
int mcrt_scene_texels(mcrt_scene* scene, int* n_texels);

/* ---- light layers and bake under extra lights: one visibility and one direct plane PER LIGHT, and their sum -------------------
 * What a compositor or a skin editor needs to dim, recolour or switch off one light of a key / fill / rim set without a new
 * render.  mcrt_render_light_device, mcrt_bake_light_device & co stay as they are and go on refusing a handle with extra lights;
 * these entries take such a handle.  The handle's lights are read BY VALUE at enqueue, as a render reads them: a pass enqueued
 * before mcrt_scene_set_extra_lights keeps the lights it was enqueued with.
 * Light 0 is the scene's own light, lights 1 .. K the handle's extra lights ("extra lights"), M = MCRT_MAX_LIGHTS = 4 plane slots.
 * LIGHT LAYERS.  At the primary hit h of the pixel-centre ray of "light layers", origin o, view = normalize(o - h.point), with
 * the ONE seed of "light layers" (depth 0, one per hit, shared by all lights), S = shadow_samples:
 *   vis_k       per light k = 0 .. K.  soft_shadows && shadow_samples > 1: computeSoftShadow(h.point, h.normal, light_k, scene, S,
 *               seed) — every light sees the hit's same 2 * S draws, and light k's own radius decides between its disk and the
 *               single ray with the raw normal (a radius below 1e-4); otherwise
 *               isInShadow(h.point, normalize(h.normal), light_k.position) ? 0 : 1
 *   D_0         shade(h, view, light_0, scene, ShadingParams{}, vis_0)
 *   D_k, k >= 1 shade(h, view, light_k, scene, ShadingParams{kd, ks, ambient = 0, shininess}, vis_k); each D is clamped by shade
 *               itself, and its alpha is what shade returns: the texel's
 *   combined    rgb = clamp(((D_0.rgb + D_1.rgb) + D_2.rgb) + D_3.rgb, 0, 1), added left to right over the lights the handle
 *               has; a = D_0.a
 *   occlusion   as in "light layers": it does not read a light
 * Planes: visibility[k] = vis_k (1 float), direct[k] = D_k (4 floats), occlusion (1 float), combined (4 floats).
 * At a miss every vis_k is 1.0f, every D_k and combined (0, 0, 0, 0), occlusion 1.0f.  A plane asked for a light the handle lacks
 * (k > K) holds the miss constants everywhere — an absent light is a black light; nothing is refused for it, so a batch of
 * handles with different K is one call.
 * RECOMPOSITION (part of the contract).  For every pixel with a hit, the beauty frame of the handle with the same lights at
 * samples_per_pixel = 1, no depth of field, max_bounces = 0 and the same shadow settings
 *   - with ao_enabled = 0 EQUALS combined, bit for bit;
 *   - with ao_enabled = 1 equals k = 1.0f - ao_intensity * (1.0f - occlusion); rgb = clamp(combined.rgb * k, 0, 1); a = combined.a.
 * With K = 0, visibility[0], direct[0] and occlusion are the bytes of mcrt_render_light_device's planes, and combined is the
 * formula on D_0 alone.
 * LIGHT BAKE.  The same per sub-sample s of "light bake", with its P, N and view = N: vis_k,s, D_k,s and
 * comb_s = clamp(sum over k of D_k,s) with alpha D_0,s.a.  Every plane is the "mean" of its sub-sample values; combined is the
 * mean of comb_s, NOT the clamp of the means.  Dead texels: 1.0f / (0, 0, 0, 0); a light the handle lacks: the same.  position and
 * normal are unchanged.
 * Each family keeps the rules of its single-light entries: whole frames, asynchronous on `stream` and not into a graph being
 * recorded, no workspace, no counters and none of the handle's events, one launch per kernel and 4096 frames, a handle may be
 * listed more than once and the handles of a batch may carry different lights, the gaps between frames are not written — and the
 * same MCRT_ERR_INVALID list before any device work, the planes untouched, with "all planes NULL" meaning every pointer of the
 * struct.  The one-shot forms add the checks of mcrt_scene_set_extra_lights on `lights` / `n_lights`, right behind the NULL
 * checks.  Zero-size frames, n_frames = 0 and scenes without texels: MCRT_OK, nothing written. */
#define MCRT_MAX_LIGHTS (1 + MCRT_MAX_EXTRA_LIGHTS)
typedef struct mcrt_light_planes_multi {
    float* visibility[MCRT_MAX_LIGHTS]; /* 1 float / pixel each; any may be NULL, not all of the struct */
    float* direct[MCRT_MAX_LIGHTS];     /* 4 floats / pixel each */
    float* occlusion;
    float* combined;                    /* 4 floats / pixel */
} mcrt_light_planes_multi;
int mcrt_render_light_multi_device(mcrt_scene* scene, const mcrt_config* cfg, const mcrt_light_planes_multi* d_out, void* stream);
int mcrt_render_light_multi_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_light_planes_multi* d_out,
                                         size_t frame_stride_pixels, void* stream);
/* one-shot host form: host pointers; `lights` are the extra lights 1 .. n_lights of the pooled handle */
int mcrt_render_light_multi(const mcrt_scene_desc* scene, const mcrt_config* cfg, const mcrt_light_source* lights, int n_lights,
                            const mcrt_light_planes_multi* out, int device);
typedef struct mcrt_bake_planes_multi {
    float* position; /* any may be NULL, not all of the struct */
    float* normal;
    float* visibility[MCRT_MAX_LIGHTS];
    float* occlusion;
    float* direct[MCRT_MAX_LIGHTS];
    float* combined;
} mcrt_bake_planes_multi;
int mcrt_bake_light_multi_device(mcrt_scene* scene, const mcrt_config* cfg, int grid, const mcrt_bake_planes_multi* d_out, void* stream);
int mcrt_bake_light_multi_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, int grid,
                                       const mcrt_bake_planes_multi* d_out, size_t texel_stride, void* stream);
int mcrt_bake_light_multi(const mcrt_scene_desc* scene, const mcrt_config* cfg, const mcrt_light_source* lights, int n_lights, int grid,
                          const mcrt_bake_planes_multi* out, int device);

/* ---- skins on resident scenes: a new skin for a scene that is already on the device -----------------------------------------
 * Everything in a flattened skin scene but its texels is a function of pose, camera and light alone.  A REPAINTABLE handle takes
 * a new skin from a 64 x skin_height RGBA8 image in device memory with one small kernel — no scene build, no flattening, no upload
 * of the blob — and one launch repaints a whole batch of handles.
 * A repaintable handle ALWAYS holds the full mesh table of its skin kind, the one mcrt_skin_texel describes: 12 meshes for a
 * 64x64 skin, 7 for a 64x32 one.  mcrt_build_skin_scene (like the reference's MeshBuilder::buildScene) drops an outer part whose
 * texels are all transparent; here that part stays, with its texels at alpha 0.  The frames are the same bit for bit: an outer
 * box whose texels all have alpha 0 never produces a hit (intersection.cpp:311-360 finds the entry and the exit face transparent
 * and returns a miss, and intersectScene keeps only hits).  The id layer's mesh index of such a handle therefore always follows
 * mcrt_skin_texel's table: the "later meshes move up" caveat there does not apply.
 *
 * mcrt_scene_create_skin: the builder's figure for skin_height 64 or 32 at `pose` (NULL: pose 0) with every part present.  Of
 * `look` (NULL: the builder's defaults) the light, camera and background fields are copied; its meshes and textures are ignored.
 * Until the first repaint the texels are those of an all-(255,255,255,255) skin.  The handle is an ordinary mcrt_scene for every
 * other call. */
int mcrt_scene_create_skin(int skin_height, const float pose[12], const mcrt_scene_desc* look, int device, mcrt_scene** out);
/* Repaints the handle from d_skin_rgba8: 64 * skin_height * 4 bytes of DEVICE memory, row-major, aligned to at least 4 bytes.
 * Asynchronous on `stream` (not into a graph being recorded on it).  Afterwards the resident blob is byte for byte what
 * mcrt_scene_flatten gives for the full-table scene with that skin's texels: texel = u8 / 255.0f (the floats are formed on the
 * host), the alpha predicate words, and MESH_OPAQUE on a mesh iff none of its texels has alpha 0.
 * Ordering: the repaint waits for the handle's earlier renders (mcrt_render_device[_ex], its frame of mcrt_render_batch_device)
 * and earlier repaints, and the handle's next render waits for the repaint, whatever streams they are given — the handle's event
 * chain, as for mcrt_render_batch_device.  Layers, ground and pick passes of the handle take none of its events: ordering THOSE
 * against a repaint (stream order, or an event of the caller's) is the caller's job. */
int mcrt_scene_set_skin_device(mcrt_scene* scene, const uint8_t* d_skin_rgba8, void* stream);
/* One launch repaints n handles; skin i starts at d_skins + i * skin_stride_bytes.  The stride is at least the image size and a
 * multiple of 4.  The handles take images of one size — 64x64 classic and 64x64 slim handles (mcrt_scene_create_skin_model) may
 * be mixed freely, the launch chooses each workgroup's tables by its handle; 64x64 with 64x32 may not — and are on one device,
 * none listed twice.  n = 0: MCRT_OK, nothing done. */
int mcrt_scene_set_skins_batch_device(mcrt_scene* const* scenes, int n, const uint8_t* d_skins, size_t skin_stride_bytes, void* stream);
/* The host form: uploads the 16 KB (8 KB) image from HOST memory and repaints, synchronously. */
int mcrt_scene_set_skin(mcrt_scene* scene, const uint8_t* skin_rgba8);
/* Host only.  For each texel of the full-table figure's pool, in pool order (meshes, their face slots 0..5, a face's texels
 * row-major), the skin pixel index y * 64 + x the texel is cut from, by the tables of mcrt_skin_texel (a legacy skin's mirrored
 * limbs included).  Returns the count — 3264 for skin_height 64, 2016 for 32 — and writes min(count, capacity) entries. */
int mcrt_skin_pool_map(int skin_height, int32_t* out, int capacity);
/* MCRT_ERR_INVALID, before any device work: a NULL handle, entry, image or `out`; a skin_height other than 64 or 32; n < 0; a
 * stride that is no multiple of 4 or smaller than the image; an image that is not 4-byte aligned; a handle that
 * mcrt_scene_create_skin did not create; handles of different image sizes or devices in one batch; a handle listed twice. */

/* ---- views of resident scenes: another pose, camera or light for a scene that is already on the device ----------------------
 * The part of a repaintable handle's blob that pose, camera, light and background decide is its prefix [header][mesh table] —
 * 2 496 bytes for a 64x64 skin, 1 536 for a 64x32 one; the texel pool, the alpha words and the owner faces of a bake behind it
 * do not depend on the view.  A view change flattens that prefix on the host, with the flattener's own code and without
 * reading a texel, and one small kernel writes it over the resident blob, keeping the one thing in it the skin owns: the
 * MESH_OPAQUE bit of every mesh.  No scene build with textures, no upload of the blob, no new handle, no repaint.
 * DEFINITION: after a view change the handle is indistinguishable from a fresh mcrt_scene_create_skin(kind, pose, look) that
 * was repainted with the handle's current skin — its blob is byte for byte mcrt_scene_flatten of the full-table scene, and
 * every frame, layer, pick, ground, reflection, light and bake result follows bit for bit.  Before the first repaint that is
 * the white figure at the new view.
 * pose NULL: the handle keeps its pose; look NULL: it keeps its look (as created, or as last set).  Both are HOST memory, read
 * before the call returns; of a look the fields mcrt_scene_create_skin reads are read, its meshes and textures are ignored.
 * Ordering: exactly a repaint's.  The view change waits for the handle's earlier renders, repaints and view changes, and the
 * handle's next render waits for it, whatever streams they are given (the handle's event chain); the library's recorded
 * launch graphs are replayed only where the render's parameters still hold.  Layers, ground, reflection, light, bake and pick
 * passes take none of the handle's events: ordering THOSE against a view change (stream order, or an event of the caller's)
 * is the caller's job, as for a repaint.
 * mcrt_scene_set_view is synchronous; the _device forms are asynchronous on `stream` (not into a graph being recorded on it). */
int mcrt_scene_set_view(mcrt_scene* scene, const float pose[12], const mcrt_scene_desc* look);
int mcrt_scene_set_view_device(mcrt_scene* scene, const float pose[12], const mcrt_scene_desc* look, void* stream);
/* One launch gives n handles their views: poses[i], looks[i].  `poses` NULL, `looks` NULL or an entry looks[i] NULL: keep.  The
 * tables travel in one asynchronous copy.  The handles take images of one size (classic and slim 64x64 handles may be mixed: each
 * table is flattened for its handle's model), are on one device, none listed twice.  n = 0: MCRT_OK. */
int mcrt_scene_set_views_batch_device(mcrt_scene* const* scenes, int n, const float (*poses)[12],
                                      const mcrt_scene_desc* const* looks, void* stream);
/* Host only, no device.  The view-dependent prefix [0, texel_offset) of the blob of mcrt_scene_create_skin(skin_height, pose,
 * look) — the white figure's, so with MESH_OPAQUE on every mesh; NULL: the builder's own pose or look.  Returns its byte count
 * (0 and the error text for a skin_height other than 64 or 32) and copies min(count, capacity) bytes into `out` (may be NULL). */
int mcrt_skin_view_table(int skin_height, const float pose[12], const mcrt_scene_desc* look, void* out, size_t capacity);
/* MCRT_ERR_INVALID, before any device work and with the blobs and the handles' state untouched: a NULL handle, `scenes` or
 * entry; n < 0; a handle that mcrt_scene_create_skin did not create; handles of different image sizes or devices in one batch; a
 * handle listed twice; a stream that is being captured. */

/* ---- studio shot: the figure on a page, with its ground shadow and its floor reflection, as ONE finished image ---------------
 * The transparent figure, the ground shadow and the ground reflection are layers for a compositor; this is that compositor, on
 * the device: one call takes a scene — or n of them — to the finished RGBA8 image (or float frame, or PNG), and one image of
 * 4 bytes per pixel leaves the card instead of float planes of 16 + 4 + 16 + 4.
 * DEFINITION.  Per pixel, four quantities enter:
 *   F       the MCRT_BACKGROUND_TRANSPARENT frame of cfg: the full beauty render — samples per pixel, depth of field, ambient
 *           occlusion, bounces — in straight alpha
 *   vis     the ground pass's visibility at ground_y (1.0f where the plane is not reached)
 *   R, dR   the reflection pass's rgba and distance at ground_y ((0, 0, 0, 0) and FLT_MAX without a reflected hit)
 *   pg      the page colour: page_color (MCRT_PAGE_COLOR), or RayTracer::backgroundColor(scene, u, v, &cfg).rgb at the pixel
 *           centre u = (px + 0.5f) / width, v = (py + 0.5f) / height (MCRT_PAGE_REFERENCE; raytracer.cpp:16-34): cfg's
 *           gradient, or scene.backgroundColor when gradient_bg is 0
 * With s = shadow_strength, k = reflectivity, fade = reflection_fade, all arithmetic float32, one rounding per operation,
 * uncontracted, in the order written, the division correctly rounded:
 *   sh    = s * (1.0f - vis)
 *   f     = fade > 0 ? clamp(1.0f - dR / fade, 0, 1) : 1.0f
 *   ar    = (k * R.a) * f                                        (0 where there is no reflected hit)
 *   keep  = (1.0f - sh) * (1.0f - ar)
 *   fl.c  = pg.c * keep + R.c * ar                               c = r, g, b
 *   out.c = F.c * F.a + fl.c * (1.0f - F.a)
 *   out.a = 1.0f
 *   rgba8 = (uint8_t)(clamp(out.c, 0, 1) * 255.0f + 0.5f) per channel, the quantiser of mcrt_quantize_rgba8
 * CONSEQUENCES (part of the contract).
 *   - A pixel with F.a == 1 holds F.rgb bit for bit: every pixel whose samples all hit opaque texels keeps the reference
 *     render's rgb.
 *   - With s == 0 the ground pass is not run, and its limit on shadow_samples does not apply; with k == 0 the reflection pass
 *     is not run, and its limits on max_bounces and shadow_samples do not apply.  The image is the same bit for bit as if
 *     the passes had run: sh and ar are exactly +0 either way, and R.c * 0 adds +0.
 *   - The page under an EDGE pixel of the figure is the pixel-centre colour.  With MCRT_PAGE_REFERENCE and s = k = 0 the
 *     image therefore equals the reference frame where F.a is 0 or 1 — under one sample per pixel without depth of field,
 *     everywhere — but not at the figure's edges under several samples: there the reference blends the gradient's values at
 *     the samples' own jittered positions, the shot blends the figure's samples over the value at the centre.
 * Here the shadow is black and the page opaque (out.a = 1); a coloured shadow and a transparent page come with the _ex entries
 * below ("the shot as a cut-out"). */
#define MCRT_PAGE_COLOR 0     /* page = page_color */
#define MCRT_PAGE_REFERENCE 1 /* page = the reference's background at the pixel centre */
typedef struct mcrt_shot {
    int32_t page;           /* MCRT_PAGE_* */
    float page_color[3];    /* read with MCRT_PAGE_COLOR; finite */
    float shadow_strength;  /* s, 0..1: how dark the fully shadowed page is */
    float reflectivity;     /* k, 0..1 */
    float reflection_fade;  /* >= 0, finite: the reflection distance at which the mirror image has vanished; 0 = no fade */
} mcrt_shot;
/* MCRT_PAGE_REFERENCE, page_color white (1, 1, 1), shadow_strength 0.6, reflectivity 0.35, reflection_fade 0 */
void mcrt_shot_init(mcrt_shot* shot);

/* The blend alone, on planes the caller already has — device memory, frame i of every input in_stride_pixels pixels on, of
 * every output out_stride_pixels pixels on (both >= width * height; the pixels between frames are neither read nor written).
 * figure is required.  visibility NULL: vis = 1; reflection NULL: no mirror image; reflection_distance NULL is legal only
 * with reflection_fade == 0 (whether or not there is a reflection plane).  The inputs must not hold NaN.  The rgba planes are
 * read and written 16 bytes at a time where they lie on a 16-byte boundary and 4 bytes at a time elsewhere; the 1-float
 * planes need their natural alignment only.  Of a handle the call reads the device and — with MCRT_PAGE_REFERENCE and
 * gradient_bg 0, on the device in stream order — the scene's background colour; a handle may be listed more than once; of
 * cfg it reads width, height, tile_size (> 0, as everywhere), gradient_bg, gradient_scale, bg_center and bg_edge.  One launch
 * per 4096 frames, asynchronous on `stream`; none of the handles' events. */
typedef struct mcrt_shot_inputs {
    const float* figure;               /* 4 floats per pixel */
    const float* visibility;           /* 1 float per pixel, or NULL */
    const float* reflection;           /* 4 floats per pixel, or NULL */
    const float* reflection_distance;  /* 1 float per pixel, or NULL */
} mcrt_shot_inputs;
int mcrt_composite_shot_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_shot* shot,
                                     const mcrt_shot_inputs* d_in, size_t in_stride_pixels, float* d_out_f32, uint8_t* d_out_rgba8,
                                     size_t out_stride_pixels, void* stream);

/* Render + ground + reflection + blend.  The figure of every scene is rendered with MCRT_BACKGROUND_TRANSPARENT whatever the
 * handle's background mode is, through an override inside the call: the handle's mode is never written, other threads never
 * see another one, and it is the same afterwards.  The intermediate planes live in d_scratch, device memory of the caller's,
 * 16-byte aligned, of at least mcrt_shot_scratch_bytes(cfg, shot, n_frames) bytes (host only; 0 for a NULL argument, an
 * invalid shot, a zero-size frame or n_frames <= 0): the library allocates nothing behind the device forms.  It holds only
 * the planes the shot needs, one after the other, each for all n_frames frames (width * height pixels apart) and each
 * starting on a 16-byte boundary:
 *     figure 16 B/px   reflection rgba 16 B/px if k > 0   visibility 4 B/px if s > 0   reflection distance 4 B/px if k > 0 && fade > 0
 * ORDERING.  Everything is enqueued on `stream`, in order: the batched render (each handle's event chain as for
 * mcrt_render_batch_device: it waits for the handle's earlier renders, repaints and view changes, and the handle's next
 * render waits for it), the ground pass, the reflection pass, the blend.  So a shot enqueued behind
 * mcrt_scene_set_skin_device / mcrt_scene_set_view_device on the same stream shows the new skin and view without a
 * synchronisation.  Nothing is forked onto internal streams beside the render.  ground_y: n_frames heights in HOST memory,
 * read before the call returns.  Frame i lands at d_out_f32 + i * frame_stride_pixels * 4 floats and / or d_out_rgba8 +
 * i * frame_stride_pixels * 4 bytes.
 * MCRT_ERR_INVALID, before any device work, with outputs and scratch untouched: a NULL argument (cfg, shot, the array, an
 * entry, ground_y); n_frames < 0; a page other than the two constants; shadow_strength or reflectivity outside [0, 1] or NaN;
 * a reflection_fade that is negative or not finite; a page colour that is not finite; a ground_y that is not finite; both
 * outputs NULL; a handle listed twice (each owns one workspace); max_bounces > 4000; soft_shadows && shadow_samples > 113
 * when s > 0 or k > 0; max_bounces > 8 when k > 0; a frame of 2^31 pixels or more; a stride below width * height; scratch
 * NULL, too small or not 16-byte aligned; handles on different devices; a stream that is being captured (shots are not
 * recorded into a caller's graph).  The composite call refuses what applies to it: the NULL arguments (figure included), the
 * shot's fields, reflection_distance NULL with reflection_fade > 0, both outputs NULL, the frame size, either stride, the
 * devices, a captured stream.  Zero-size frames (width, height or tile_size <= 0) and n_frames == 0: MCRT_OK, nothing
 * written, checked behind the argument checks above it in this list and before strides and scratch. */
size_t mcrt_shot_scratch_bytes(const mcrt_config* cfg, const mcrt_shot* shot, int n_frames);
int mcrt_render_shot_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_shot* shot,
                                  const float* ground_y, void* d_scratch, size_t scratch_bytes, float* d_out_f32, uint8_t* d_out_rgba8,
                                  size_t frame_stride_pixels, void* stream);
/* one scene, one height */
int mcrt_render_shot_device(mcrt_scene* scene, const mcrt_config* cfg, const mcrt_shot* shot, float ground_y, void* d_scratch,
                            size_t scratch_bytes, float* d_out_f32, uint8_t* d_out_rgba8, void* stream);
/* One-shot host forms: host pointers, rendered on `device` with pooled handles like mcrt_render_batch; they allocate and free
 * their own scratch.  out_rgba: n * width * height * 4 floats and / or out_rgba8: as many bytes, frame after frame. */
int mcrt_render_shot(const mcrt_scene_desc* scene, const mcrt_config* cfg, const mcrt_shot* shot, float ground_y, float* out_rgba,
                     uint8_t* out_rgba8, int device);
int mcrt_render_shot_batch(const mcrt_scene_desc* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_shot* shot,
                           const float* ground_y, float* out_rgba, uint8_t* out_rgba8, int device);
/* mcrt_render_shot's RGBA8 image as a PNG (colour type 6, alpha 255 everywhere); a zero-size frame: MCRT_ERR_INVALID, as
 * for mcrt_render_png */
int mcrt_render_shot_png(const mcrt_scene_desc* scene, const mcrt_config* cfg, const mcrt_shot* shot, float ground_y, const char* path,
                         int device);

/* The shot with a FLOOR-OCCLUSION term.  A strength o = floor_occlusion in [0, 1] and the ground-occlusion pass's plane occ
 * (1.0f where the plane is absent) enter the blend between the shadow and the reflection; everything else is as above:
 *   oc    = o * (1.0f - occ)
 *   keep  = ((1.0f - sh) * (1.0f - oc)) * (1.0f - ar)
 * CONSEQUENCE.  With o == 0, or without an occlusion plane, oc is +0 and (1 - sh) * 1.0f is (1 - sh) exactly: the image is
 * the one of the entries above bit for bit, the ground-occlusion pass is not run, and its limits on ao_samples / ao_radius
 * do not apply.  The entries above are these with o = 0 and no plane; mcrt_shot and mcrt_shot_inputs are unchanged.
 * The floor's sampling is cfg's ao_samples / ao_radius — the fields the figure's own ambient occlusion reads when ao_enabled.
 *   mcrt_shot_scratch_bytes_occ        the layout above, and behind it an occlusion plane of 4 B/px when o > 0 (the offsets of
 *                                      the other planes do not move); 0 also for an o outside [0, 1] or NaN
 *   mcrt_render_shot_batch_device_occ  render, ground, reflection, ground occlusion, blend, in that order on `stream`; the
 *                                      event rules and argument checks of mcrt_render_shot_batch_device, and MCRT_ERR_INVALID
 *                                      also for a floor_occlusion outside [0, 1] or NaN and, with o > 0, for ao_samples < 1,
 *                                      ao_samples > 113 or an ao_radius that is not finite
 *   mcrt_composite_shot_batch_device_occ   the blend alone; d_occlusion: 1 float per pixel, frame i in_stride_pixels pixels
 *                                      on, or NULL; it refuses a floor_occlusion outside [0, 1] or NaN
 *   mcrt_render_shot_batch_occ, mcrt_render_shot_png_occ   the host forms */
size_t mcrt_shot_scratch_bytes_occ(const mcrt_config* cfg, const mcrt_shot* shot, float floor_occlusion, int n_frames);
int mcrt_render_shot_batch_device_occ(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_shot* shot,
                                      float floor_occlusion, const float* ground_y, void* d_scratch, size_t scratch_bytes, float* d_out_f32,
                                      uint8_t* d_out_rgba8, size_t frame_stride_pixels, void* stream);
int mcrt_composite_shot_batch_device_occ(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_shot* shot,
                                         const mcrt_shot_inputs* d_in, const float* d_occlusion, float floor_occlusion, size_t in_stride_pixels,
                                         float* d_out_f32, uint8_t* d_out_rgba8, size_t out_stride_pixels, void* stream);
int mcrt_render_shot_batch_occ(const mcrt_scene_desc* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_shot* shot,
                               float floor_occlusion, const float* ground_y, float* out_rgba, uint8_t* out_rgba8, int device);
int mcrt_render_shot_png_occ(const mcrt_scene_desc* scene, const mcrt_config* cfg, const mcrt_shot* shot, float floor_occlusion, float ground_y,
                             const char* path, int device);

/* The shot as a CUT-OUT, with a shadow colour and crop bounds.  One straight-alpha RGBA image holds figure, shadow, occlusion
 * and reflection; composited over any page it gives what the opaque shot gives for that page.  New are a page mode,
 * MCRT_PAGE_TRANSPARENT (only the _ex entries accept it; the entries above keep refusing every page but 0 and 1), and a shadow
 * colour C = shadow_color[3], finite, default (0, 0, 0), which the floor-occlusion darkening uses too.
 * DEFINITION.  The inputs F, vis, R, dR, pg, occ and the settings s, k, fade, o are those above.  All arithmetic float32, one
 * rounding per operation, uncontracted, in the order written, divisions correctly rounded:
 *   sh   = s * (1.0f - vis)
 *   f    = fade > 0 ? clamp(1.0f - dR / fade, 0, 1) : 1.0f
 *   ar   = (k * R.a) * f
 *   oc   = o * (1.0f - occ)                      (multiplied in only where there is an occlusion plane, as above)
 *   lit  = (1.0f - sh) * (1.0f - oc)
 *   keep = lit * (1.0f - ar)                     (the keep above, same bits)
 *   dk   = (1.0f - lit) * (1.0f - ar)            (the weight of the shadow colour)
 * OPAQUE PAGES (MCRT_PAGE_COLOR, MCRT_PAGE_REFERENCE):
 *   fl.c  = (pg.c * keep + C.c * dk) + R.c * ar
 *   out.c = F.c * F.a + fl.c * (1.0f - F.a)
 *   out.a = 1.0f
 * When all three channels of C compare equal to 0 the C term is not formed at all: fl.c = pg.c * keep + R.c * ar, and the
 * result is byte for byte that of the _occ entries with the same settings, signs of zero included.
 * TRANSPARENT PAGE:
 *   af   = 1.0f - keep                           (the floor's alpha)
 *   fp.c = C.c * dk + R.c * ar                   (the floor's colour, premultiplied; C = 0: fp.c = R.c * ar)
 *   u    = 1.0f - F.a
 *   if af == 0:   out = F                        (all four channels as they are)
 *   else:         A = F.a + af * u
 *                 out.a = A
 *                 out.c = A > 0 ? (F.c * F.a + fp.c * u) / A : 0      (A <= 0: out = (0, 0, 0, 0))
 * The RGBA8 plane quantises all four channels with the quantiser of mcrt_quantize_rgba8; out.c may exceed 1 at alphas near
 * one float ulp, and the quantiser clamps it.  The page evaluation (the reference's background, page_color) is not read with
 * the transparent page; a page_color that is not finite is refused all the same.
 * CONSEQUENCES (part of the contract).
 *   - With s = k = o = 0, or with the planes absent, af is exactly +0 and the image is the MCRT_BACKGROUND_TRANSPARENT render
 *     itself, bit for bit; the passes are not run and their limits on shadow_samples, max_bounces, ao_samples and ao_radius
 *     do not apply.
 *   - A pixel with F.a == 1 holds F.rgb and alpha 1 (a channel that is -0 in F may come out +0).
 *   - A pixel with no figure and nothing on the floor is F, so (0, 0, 0, 0); one with a black shadow only is (0, 0, 0, af).
 *   - OVER ANY PAGE.  For a finite pg, out.c * out.a + pg.c * (1 - out.a) equals the opaque shot's out.c for that page up to
 *     rounding — in exact arithmetic they are one expression, 1 - A = u * keep: within 16 * 2^-24 in float and one level in
 *     RGBA8.
 *   - A straight-alpha 8-bit image cannot carry colour precision at alphas that quantise to 0 or 1 level: a property of the
 *     format (PNG's colour type 6), not of this blend.  Compositors that need it take the float plane.
 * BOUNDS, only with the transparent page: d_bounds, optional, one int32[4] per frame: {x0, y0, x1, y1}, x0 and y0 the minima
 * of x and y over the pixels with float out.a > 0.0f, x1 and y1 the maxima of x + 1 and y + 1 over them; a frame without such
 * a pixel gets {width, height, 0, 0}.  The set is a superset of the pixels whose 8-bit alpha is above 0.  The call writes
 * every entry completely (the caller initialises nothing; 4-byte alignment); the result is valid in stream order behind the
 * blend.  Zero-size frames and n_frames == 0 write nothing.
 * ENTRIES.  Ordering, events, scratch and argument checks are those of the _occ entries, in the same order;
 * mcrt_shot_scratch_bytes_ex has the layout and sizes of mcrt_shot_scratch_bytes_occ for the same s, k, fade and o.
 * MCRT_ERR_INVALID before any device work also for: a page outside 0..2; a shadow_color that is not finite; a non-NULL bounds
 * pointer, a non-zero crop or a non-NULL out_bounds with an opaque page.
 * mcrt_render_shot_png_ex writes colour type 6 with the image's real alpha; crop != 0 writes only the bounds rectangle — an
 * empty rectangle writes the whole frame, so the call never fails for an all-transparent skin — and out_bounds (int32[4] or
 * NULL) receives the rectangle either way. */
#define MCRT_PAGE_TRANSPARENT 2 /* no page: the shot as a straight-alpha cut-out (the _ex entries only) */
typedef struct mcrt_shot_ex {
    mcrt_shot shot;         /* page may also be MCRT_PAGE_TRANSPARENT */
    float floor_occlusion;  /* o */
    float shadow_color[3];  /* C, finite */
} mcrt_shot_ex;
/* mcrt_shot_init, o = 0, C = (0, 0, 0); NULL is ignored */
void mcrt_shot_ex_init(mcrt_shot_ex* shot);
size_t mcrt_shot_scratch_bytes_ex(const mcrt_config* cfg, const mcrt_shot_ex* shot, int n_frames);
int mcrt_composite_shot_batch_device_ex(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_shot_ex* shot,
                                        const mcrt_shot_inputs* d_in, const float* d_occlusion, size_t in_stride_pixels, float* d_out_f32,
                                        uint8_t* d_out_rgba8, size_t out_stride_pixels, int32_t (*d_bounds)[4], void* stream);
int mcrt_render_shot_batch_device_ex(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_shot_ex* shot,
                                     const float* ground_y, void* d_scratch, size_t scratch_bytes, float* d_out_f32, uint8_t* d_out_rgba8,
                                     size_t frame_stride_pixels, int32_t (*d_bounds)[4], void* stream);
/* host form: out_bounds NULL or n_frames entries in host memory */
int mcrt_render_shot_batch_ex(const mcrt_scene_desc* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_shot_ex* shot,
                              const float* ground_y, float* out_rgba, uint8_t* out_rgba8, int32_t (*out_bounds)[4], int device);
int mcrt_render_shot_png_ex(const mcrt_scene_desc* scene, const mcrt_config* cfg, const mcrt_shot_ex* shot, float ground_y, const char* path,
                            int crop, int32_t* out_bounds, int device);

/* number of pixel rows owned by (first, step) and therefore the packed buffer height */
int mcrt_owned_pixel_rows(const mcrt_config* cfg, int tile_row_first, int tile_row_step);

/* Scatter one rank's packed rows (as produced with MCRT_LAYOUT_PACKED) into a full frame.
 * Used by the gather root after the RCCL gather. */
int mcrt_unpack_rows_device(const mcrt_config* cfg, int tile_row_first, int tile_row_step,
                            const float* d_packed, float* d_frame, void* stream);

/* The same for all ranks of a gather in one launch: d_gathered holds `world` packed buffers (rank r
 * rendered with first=r, step=world), rank_stride_pixels float4 apart (>= the padded packed size
 * ceil(tile_rows/world) * tile_size * width). */
int mcrt_assemble_frame_device(const mcrt_config* cfg, int world, const float* d_gathered, size_t rank_stride_pixels,
                               float* d_frame, void* stream);

/* float RGBA → RGBA8, `(uint8_t)(clamp(c,0,1)*255.0f+0.5f)` per channel
 * (/root/reference/src/output/image_writer.cpp:18-22 ≡ src/skin/image.cpp:31-36). */
int mcrt_quantize_rgba8_device(const float* d_rgba, uint8_t* d_out, size_t n_pixels, void* stream);
void mcrt_quantize_rgba8(const float* rgba, uint8_t* out, size_t n_pixels);

/* ---- PNG hand-off (the step after the path: ImageWriter::writePNG, image_writer.cpp:6-28) -------- */
/* Writes an 8-bit RGBA PNG (colour type 6, no interlace, filter 0, zlib *stored* blocks: no
 * compression, bounded by memory bandwidth).  Any PNG reader decodes it to the same pixels the
 * reference's stbi_write_png output decodes to.  Returns MCRT_OK or MCRT_ERR_INVALID (bad
 * arguments, or the file cannot be created / written — writePNG's `false`). */
int mcrt_write_png_rgba8(const char* path, const uint8_t* rgba, int width, int height);
/* In-memory form: returns the PNG size; writes it when `capacity` suffices. */
size_t mcrt_encode_png_rgba8(const uint8_t* rgba, int width, int height, uint8_t* out, size_t capacity);
/* Quantise a float RGBA image exactly like ImageWriter::writePNG and write it. */
int mcrt_write_png_f32(const char* path, const float* rgba, int width, int height);
/* TileRenderer::render + ImageWriter::writePNG in one call: render on `device` (an index, or MCRT_DEVICE_ALL), quantise
 * in the kernel epilogue, copy 4 B/pixel back (mcrt_render_rgba8), write the file.  Invalid frame sizes write nothing and
 * return MCRT_ERR_INVALID (writePNG rejects empty images, image_writer.cpp:7-9). */
int mcrt_render_png(const mcrt_scene_desc* scene, const mcrt_config* cfg, const char* path, int device);

/* timings of the last mcrt_render() / mcrt_render_multi() on this thread, milliseconds: flatten_ms — scene
 * flattening on the host; h2d_ms — uploads, workspace checks and every launch call; kernel_ms — rank 0's
 * pipeline on its device (hipEvents); d2h_ms — from the last launch call until the last row has landed
 * (it overlaps the render); total_ms — the whole call */
typedef struct mcrt_timings {
    float flatten_ms, h2d_ms, kernel_ms, d2h_ms, total_ms;
} mcrt_timings;
int mcrt_last_timings(mcrt_timings* out);

/* Device-only timing helper used by bench.py: enqueues `iters` renders of the given shard on
 * `stream`, each bracketed by hipEvents recorded on that same stream and waited for, and returns
 * the average duration in ms of one render's whole pipeline (every lane and kernel of the frame). */
int mcrt_time_render_device(mcrt_scene* scene, const mcrt_config* cfg, int tile_row_first,
                            int tile_row_step, int out_layout, float* d_out_rgba, void* stream,
                            int iters, float* avg_render_ms);

/* ---- scene construction helpers (MeshBuilder / SkinParser layout) -------
 * Build the reference's character scene from an RGBA8 skin image (64x64 or 64x32), exactly as
 * SkinParser::parse (skin_parser.cpp:11-132, texel = u8/255.0f per image.cpp:16-21) followed by
 * MeshBuilder::buildScene (mesh_builder.cpp:145-202) would.  pose = 12 floats:
 * {head, body, rightArm, leftArm, rightLeg, leftLeg} x {rotX, rotZ} degrees (pose.h:9-22).
 * The returned description owns its arrays; free with mcrt_scene_desc_free(). */
int mcrt_build_skin_scene(const uint8_t* skin_rgba8, int skin_width, int skin_height,
                          const float pose[12], mcrt_scene_desc** out);
/* ---- player models.  MCRT_SKIN_CLASSIC is the reference's figure, arms 4 texels wide, and what every entry without a model
 * argument means.  MCRT_SKIN_SLIM is Minecraft's slim ("Alex") model, for 64x64 skins only: it differs in the four arm boxes
 * and nowhere else.  Their unwrap boxes {ox, oy, w, h, d} are {40,16,3,12,4} (right arm), {32,48,3,12,4} (left arm),
 * {40,32,3,12,4} and {48,48,3,12,4} (their outer layers) — front and back 3x12, top and bottom 3x4, sides 4x12 — and the
 * arm is the box of size {3, 12, 4} at {-+5.5, 18, 0}, x = -7 .. -4 and 4 .. 7, flush with the body as the classic arm is,
 * rotated about the pivot {-+5.5, 24, 0} on its own axis; the outer layer's offset stays 0.5 and the mesh order is classic's.
 * A slim figure with every part present has 12 meshes, 72 textures, 3264 - 4 * 32 = 3136 pool texels and 196 alpha words;
 * its blob prefix [header][mesh table] has classic's 2496 bytes.  Every `_model` entry with MCRT_SKIN_CLASSIC is exactly
 * its entry without; a model other than these two, or slim with skin_height 32, is MCRT_ERR_INVALID. */
#define MCRT_SKIN_CLASSIC 0
#define MCRT_SKIN_SLIM 1
int mcrt_build_skin_scene_model(const uint8_t* skin_rgba8, int skin_width, int skin_height, int model,
                                const float pose[12], mcrt_scene_desc** out);
int mcrt_scene_create_skin_model(int skin_height, int model, const float pose[12], const mcrt_scene_desc* look, int device, mcrt_scene** out);
int mcrt_skin_texel_model(int skin_height, int model, int mesh, int face_slot, int tx, int ty, int* skin_x, int* skin_y);
int mcrt_skin_pool_map_model(int skin_height, int model, int32_t* out, int capacity); /* 3136 entries for slim */
int mcrt_skin_view_table_model(int skin_height, int model, const float pose[12], const mcrt_scene_desc* look, void* out, size_t capacity);
/* Host only.  Which model a skin image was painted for, by the rule the common skin viewers use — a HEURISTIC, since the image
 * itself does not say: MCRT_SKIN_SLIM for a 64x64 image whose 64 pixels in the rectangles (x, y, w, h) = (50,16,2,4),
 * (54,20,2,12), (42,48,2,4) and (46,52,2,12) — columns of the inner arms that a slim unwrap leaves unused — all have alpha 0,
 * MCRT_SKIN_CLASSIC for every other 64x64 or 64x32 image.  A classic skin with transparent arms reads as slim; a slim skin
 * whose painter filled those columns reads as classic.  -1 and the error text for NULL or another size. */
int mcrt_skin_model_of(const uint8_t* skin_rgba8, int skin_width, int skin_height);
/* ---- capes.  A cape is a second image, RGBA8 and exactly 64x32 (HD and animated capes: no), unwrapped as Minecraft unwraps
 * it: the box {ox, oy, w, h, d} = {0, 0, 10, 16, 1}, 372 texels inside the image's 22x17 corner, (0,0) and (21,0) unread.
 * The mesh is the box of size {10, 16, 1} at {0, 16, -2.5} — x -5 .. 5, y 8 .. 24, z -3 .. -2, on the body's back (the figure
 * faces +z) — with no outer-layer offset, hinged at the pivot {0, 24, -2} by rot_x = cape_angle degrees, rot_z = 0: a positive
 * angle moves the hem towards -z, away from the legs.  cape_angle is accepted within 0 .. 90 (10 is the usual rest angle);
 * NaN or a value outside is MCRT_ERR_INVALID; below 0.01 degrees the box is unposed, as any part is.  The cape does NOT follow
 * the body part's own rotation: a mesh has one pivot, and the built-in poses turn the body by 5 degrees at the most.
 * The box is turned half a turn about y, as Minecraft's cape model is, so the face slots (0 back = -z, 1 front = +z, 2 left =
 * +x, 3 right = -x, 4 top, 5 bottom) are cut from (x, y, w, h) = (1,1,10,16) — the outward face, seen from behind the player —
 * (12,1,10,16), (11,1,1,16), (0,1,1,16), and (1,0,10,1) and (11,0,10,1) each read turned half a turn, texel (tx, ty) from
 * (w-1-tx, h-1-ty).  Seen from behind (camera on the -z side, the viewer's left is +x) image column 1 lies at the +x edge and
 * row 1 at the hinge: the picture reads as painted.
 * The cape is the LAST mesh of its figure: index 12 of a full 64x64 table (classic or slim), 7 of a 64x32 one.  A cape whose
 * 372 texels all have alpha 0 is dropped, as a fully transparent outer part is; cape_rgba8 NULL is the entry without a cape,
 * byte for byte (the angle is then not read). */
int mcrt_build_skin_scene_cape(const uint8_t* skin_rgba8, int skin_width, int skin_height, int model, const float pose[12],
                               const uint8_t* cape_rgba8 /* 64x32, or NULL */, float cape_angle, mcrt_scene_desc** out);
/* Host only.  The cape pixel (x, y) that texel (tx, ty) of face `face_slot` of the cape mesh is cut from; and the cape mesh's
 * 372 texels in pool order — six faces in slot order, row-major — as pixel indices y * 64 + x (returns the count, copies
 * min(count, capacity)).  mcrt_skin_texel[_model] keeps refusing the cape's mesh index: this is the cape's mapping. */
int mcrt_cape_texel(int face_slot, int tx, int ty, int* cape_x, int* cape_y);
int mcrt_cape_pool_map(int32_t* out, int capacity);
/* A repaintable handle WITH a cape mesh: mcrt_scene_create_skin_model's figure plus the cape at cape_angle, 13 or 8 meshes, a
 * prefix of 2688 or 1728 bytes, the skin's pool texels and then the cape's 372, whose 24 alpha-predicate words are its own.
 * A fresh handle holds a white skin and a TRANSPARENT cape (its mesh's opaque flag clear: it is never hit).  Every entry that
 * takes a repaintable handle takes a caped one; mcrt_scene_set_skin* leave the cape's texels, words and flag alone, and
 * mcrt_scene_set_cape* the skin's.  The handles of one batch call (set_skins, set_views, set_capes) are all caped or all
 * capeless. */
int mcrt_scene_create_skin_cape(int skin_height, int model, const float pose[12], const mcrt_scene_desc* look, float cape_angle, int device, mcrt_scene** out);
/* Repaint the cape of caped handles from 64x32 RGBA8 images: from host memory, synchronous; from device memory (4-byte
 * aligned), asynchronous on `stream`; and n handles in one launch, cape i at d_capes + i * cape_stride_bytes (a multiple of 4,
 * at least 8192, or 0: every handle takes the one image at d_capes).  A NULL image means a transparent cape (in the batch
 * form: every handle's).  The handle's renders are ordered against the repaint by the library, as against a skin repaint. */
int mcrt_scene_set_cape(mcrt_scene* scene, const uint8_t* cape_rgba8);
int mcrt_scene_set_cape_device(mcrt_scene* scene, const uint8_t* d_cape_rgba8, void* stream);
int mcrt_scene_set_capes_batch_device(mcrt_scene* const* scenes, int n, const uint8_t* d_capes, size_t cape_stride_bytes, void* stream);
/* The views of caped handles.  mcrt_skin_view_table_cape: mcrt_skin_view_table_model for the caped figure, 2688 or 1728
 * bytes.  mcrt_scene_set_view_cape[_device]: mcrt_scene_set_view[_device] with another cape angle (cape_angle NULL keeps the
 * handle's); the batch form takes one angle per scene (cape_angles NULL keeps them all).  The plain view entries on a caped
 * handle keep its angle.  A cape angle for a capeless handle is MCRT_ERR_INVALID. */
int mcrt_skin_view_table_cape(int skin_height, int model, const float pose[12], const mcrt_scene_desc* look, float cape_angle, void* out, size_t capacity);
int mcrt_scene_set_view_cape(mcrt_scene* scene, const float pose[12], const mcrt_scene_desc* look, const float* cape_angle);
int mcrt_scene_set_view_cape_device(mcrt_scene* scene, const float pose[12], const mcrt_scene_desc* look, const float* cape_angle, void* stream);
int mcrt_scene_set_views_cape_batch_device(mcrt_scene* const* scenes, int n, const float (*poses)[12], const mcrt_scene_desc* const* looks,
                                           const float* cape_angles, void* stream);
/* MeshBuilder::buildDefaultScene (mesh_builder.cpp:204-223): white 1x1 textures, no outer layer */
int mcrt_build_default_scene(const float pose[12], mcrt_scene_desc** out);
/* one of the 7 built-in poses of pose.h:25-92 (index 0..6) → 12 floats; returns MCRT_ERR_INVALID
 * for other indices */
int mcrt_builtin_pose(int index, float pose_out[12]);
void mcrt_scene_desc_free(mcrt_scene_desc* desc);

/* ---- flattened blob (what actually travels to HBM) — exposed for host-only tests ---------- */
/* Serialises the flattened scene (per-mesh AABB, rotation trig, face texture table, texel pool,
 * camera basis, light) into a byte blob.  Returns the blob size; copies min(size, capacity). */
size_t mcrt_scene_flatten(const mcrt_scene_desc* desc, void* blob, size_t capacity);

/* ---- per-function device probes (GPU parity tests mirror the reference's unit tests) ------ */
typedef struct mcrt_hit {
    int32_t hit;
    float t;
    float point[3];
    float normal[3];
    float texture_color[4];
    int32_t is_outer_layer;
} mcrt_hit;

/* Waits for the device, then downloads the scene's resident blob (what mcrt_scene_flatten gave at creation, as later repaints
 * left it) into out.  Returns the blob's size in bytes — never below 192, the header's size — and copies min(size, capacity);
 * on failure an MCRT_ERR_* code (all of them below 192; a NULL argument: MCRT_ERR_INVALID). */
int mcrt_probe_scene_blob(mcrt_scene* scene, void* out, size_t capacity);
/* Waits for the device, then reads the work units that the last pass of the handle's last render queued on its first lane:
 * per unit its record (4 x uint32: owned tile | block flag << 31, then a pixel range {first, end} of the tile's row-major
 * order or a block {x | y << 16, width | height << 16} inside the tile, then its first sample slot) and its primary hits.
 * Returns the number of units and copies min(units, capacity) entries into each array that is not NULL; 0 before the first
 * render; on failure an MCRT_ERR_* code. */
int mcrt_probe_units(mcrt_scene* scene, uint32_t* records, uint32_t* hits, int capacity);
/* intersectScene (intersection.cpp:408-421) for n rays; rays = n*6 floats (origin, direction) */
int mcrt_probe_intersect(mcrt_scene* scene, const float* rays, int n, mcrt_hit* out);
/* RayTracer::traceRay(ray, scene, depth, maxBounces, ShadingParams{}, &cfg) (raytracer.cpp:82-148)
 * for n rays; out = n*4 floats.  The handle's extra lights are ignored: the probe is the reference's own function. */
int mcrt_probe_trace(mcrt_scene* scene, const mcrt_config* cfg, const float* rays, int n, int depth,
                     float* out_rgba);
/* first n outputs of uniform_real_distribution<float>(0,1) over std::mt19937(seed) for each seed */
int mcrt_probe_mt_uniform(int device, const uint32_t* seeds, int n_seeds, int n_draws, float* out);
/* The rows of the device's sample table ("Sample table" above) for n seeds in -2^22 .. 2^22-1: out = n x 8 x 4 floats,
 * {cos, sin, sqrt, 0} per sample.  Builds the table if the device has none yet; MCRT_ERR_INVALID for a seed outside the
 * window, MCRT_ERR_HIP where there is no table (MCRT_SAMPLE_TABLE=0, no room). */
int mcrt_probe_sample_rows(int device, const int32_t* seeds, int n, float* out);
/* The words of a seed table for n seeds, out[i] = state word 397 of std::mt19937's seeding of seeds[i] as the table holds it.
 * which = MCRT_TABLE_WINDOW: seeds -2^24 .. 2^24-1 in two's complement, MCRT_ERR_INVALID for one outside; MCRT_TABLE_FULL:
 * any seed.  Builds the table if the device has none yet and lets go of it afterwards (mcrt_trim() frees a table nobody
 * holds); MCRT_ERR_HIP where there is no table (its knob at 0, no room). */
int mcrt_probe_seed_words(int device, int which, const uint32_t* seeds, int n, uint32_t* out);
/* device detmath: op 0 = sinf, 1 = cosf, 2 = powf(x, y), 3 / 4 = sin / cos output of the fused
 * mcrt_sincosf, 5 = the kernels' 3-instruction reciprocal (reference: IEEE 1.0f / x), over n inputs */
int mcrt_probe_detmath(int device, int op, const float* x, const float* y, size_t n, float* out);
/* device detmath range check against the host build of the same header:
 * op 0/1: all floats with bit patterns in [lo_bits, hi_bits]; op 2: powf(x, y0).
 * Returns the number of mismatching inputs in *mismatches (host side is multi-threaded). */
int mcrt_probe_detmath_range(int device, int op, uint32_t lo_bits, uint32_t hi_bits, float y0,
                             uint64_t* mismatches);
/* div_frame — the frame-constant division of the sample coordinates (rt_core.h) — against the general division on the
 * device, for the integer divisors d_first .. d_first + d_count - 1 and every float a sample coordinate can take
 * (0 and 2^-33 .. d + 1); mode 1 checks the form with a second correction, mode 2 the uncorrected product (the probe's
 * own check); mode 3: rt::sqrt_pos against sqrtf for 0 and every float from 2^-96 to infinity; mode 4: the device's 1.0f / d
 * against the host's (the reciprocals the probe — like the render kernels — uses are the HOST's).  tools/gpu_verify_div.py */
int mcrt_probe_div_const(int device, uint32_t d_first, uint32_t d_count, int mode, uint64_t* mismatches, uint32_t* a_failing_divisor);

#ifdef __cplusplus
}
#endif
#endif /* MCRT_H */
