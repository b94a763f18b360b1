// kernels.h — interface between the C-ABI host code (api.cpp, render_enqueue.cpp, device_stores.cpp, probes.cpp), the host
// planning (render_plan.cpp) and the HIP kernels' launchers (render_kernels.hip, pass_kernels.hip, util_kernels.hip).
// Plain structs, no HIP types in the signatures beyond hipStream_t.
#ifndef MCRT_KERNELS_H
#define MCRT_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "launch_shapes.h"
#include "mcrt.h"

namespace mcrt {

// Which tile rows of the frame a launch owns: rows first, first+step, ...
struct Shard {
    int first;
    int step;
    int tiles_x;     // tile columns
    int tiles_y;     // tile rows in the whole frame
    int owned_rows;  // number of tile rows owned
    // MCRT_LAYOUT_PACKED: owned row j is stored as packed tile row pack_first + j * pack_step (a lane
    // of a rank's shard writes into the rank's packed buffer; plain shards use 0 / 1)
    int pack_first;
    int pack_step;
};

// Device workspace of the wavefront pipeline (all HBM; sized for one batch of tile rows in which
// every sample may hit).  A *slot* is one sample of a tile that meshes can touch; a *record* is one hit
// of a chain (the primary hit of a sample and every reflection hit below it).
struct WaveSpace {
    float4* scol;           // [cap] per-sample colour, where the sample did not start a chain (miss, background)
    uint32_t* end;          // [cap] per sample: 0 = the colour is in `scol`; else how its chain ended:
                            //       (records of the chain << 1) | (1 = stopped at maxBounces, 0 = the last reflection ray missed)
    uint4* units;           // queued units of the tiles meshes can touch, in one of two forms (kernel_common.h, unit_pixel):
                            //       a pixel range {owned tile, first pixel, end pixel, slot base}, or
                            //       a block {owned tile | kUnitBlock, lx0 | ly0 << 16, width | height << 16, slot base}
    uint32_t* unit_hits;    // per unit: its primary hits (their records sit at the front of the unit's slot range)
    unsigned long long* tile_mask;  // per owned tile: meshes whose screen bound touches it
    float* tile_draws;      // [touched tiles (bg_in_plan) or all tiles of the batch][draws_stride] a tile's mt19937 draws, as uniform floats
                            // (not written and not read when the frame has a draw plate: RenderParams::draw_plate)
    uint32_t draws_stride;  // tile slots * draws_per_sample
    uint32_t unit_cap;      // capacity of `units`
    uint32_t tile_cap;      // tiles of a batch that may be touched by meshes (host-side superset of the device's culling):
                            // touched tile number k of a batch owns slots [k, k+1) * tile_slots
    // Hit records, SoA.  q_*[1] = q_*[0] + cap.
    // General variants: q_*[level & 1], ping-pong by level, every field written:
    //   q_o ray origin (.w = root = the chain's sample slot, bit-cast), q_d ray direction (.w = depth),
    //   q_p hit point, q_n hit normal (as intersectMesh returns it), q_t texel colour.
    // Flat pipeline: q_*[0] is ONE array of rec_cap records — the primary hits at their slot index (< cap), the
    // records of every deeper level densely from index cap on — in a compact form (36 B instead of 80 for an
    // un-posed scene seen through a pinhole):
    //   q_p hit point (.w = root), q_d ray direction (.w = depth | face axis << 8 | min-side << 10 | exit-face << 11),
    //   q_x texel reference of the face (the colour is fetched from the pool where the record is shaded),
    //   q_n only when the scene holds posed meshes (else the normal follows from the face code),
    //   q_o only for records below the primary hits, and for those too under depth of field (else the camera position)
    float4* q_o[2];
    float4* q_d[2];
    float4* q_p[2];
    float4* q_n[2];
    float4* q_t[2];
    int32_t* q_x;           // [rec_cap] flat pipeline: texel reference per record
    float* targets;         // [rec_cap][3*shadowSamples] light sample positions per record (level 0: reused for the AO directions)
    unsigned long long* cand;  // [rec_cap] per record: meshes its soft-shadow rays can meet (conservative first pass, once per hit)
    uint32_t* lit[2];       // [0]: [rec_cap] visible light samples per record; [1]: [cap] occluded AO samples of the primary
                            // hits (general variants: ping-pong by level parity, [cap] each)
    float4* stack;          // [stack_stride][cap] level colours of the chains, plane-major: depth d of the chain of sample slot r
                            // at [d * cap + r] — the level-0 colours of neighbouring samples share cache lines
    uint32_t* counter_base; // the counters' values when the pass began (the previous pass's `resolve` left them): a pass's counts are differences
    uint32_t* frame_info;   // [0] units of the pass, left by `primary` for `resolve`
    uint32_t* counters;     // [0] units in `units`, [1] touched tiles, [8 + L] entries of level L >= 1
                            // ([9] = level-1 records), [kCounterWords - 64] / [kCounterWords - 32] work tickets of `primary` / `lit`,
                            // [last] touched-tile bound exceeded (never, by construction; sticky);
                            // never cleared: running counts (modulo 2^32) against counter_base
    uint32_t* hit_rng;      // general variants: per-thread 624-word mt19937 states (long streams)
    uint32_t cap;           // slot capacity (= samples of the touched tiles of the largest batch)
    uint32_t tile_slots;    // slots per touched tile: min(tile, width) * min(tile, height) * spp
    int stack_stride;       // maxBounces + 1 (at least 1)
};

// Seeding std::mt19937(seed) for a hit's light samples is a 397-step sequential recurrence whose only product
// the truncated engine needs is the state word mt[397] — a pure function of the 32-bit seed.  The shadow seeds of
// a scene at the reference's scale, (unsigned)(P·(12345, 67890, 11111) + depth·99999) (raytracer.cpp:110-112),
// lie in a window around zero (|sum| < 4 M for the character scene): a table of mt[397] for the seeds
// -2^24 .. 2^24 - 1 (wrapping) is 128 MB per device, built once with the same recurrence in ~2 ms, and replaces
// the chain by one 4-byte load.  Seeds outside the window run the chain.
// integer divisors (frame widths and heights) for which rt::div_frame has been checked exhaustively against the general division
constexpr int kDivFrameMax = 16384;

constexpr uint32_t kSeedWindowHalf = 1u << 24;
constexpr uint32_t kSeedWindow = 1u << 25;  // table entries: seed s at index s + kSeedWindowHalf (mod 2^32)

// The device's sample table (DESIGN.md §4 "Sample table"): what a hit's light-disk samples are before the light enters — a pure
// function of (shadow seed, sample index).  Row r serves seed r - kSampleWindowHalf (wrapping, like the seed table) and is
// kSampleRow float4 {cs, sn, sq, 0}, one 128-byte line: d0, d1 = draws 2i, 2i+1 of std::mt19937(seed), (sn, cs) =
// mcrt_sincosf(kTwoPi * d0), sq = sqrt_pos(d1) — filled by launch_build_sample_table with the routines
// disk_sample_positions runs.  2^23 rows, 1 GiB: the seeds -2^22 .. 2^22 - 1; the built-in character's hits at the
// reference's scale stay below 3.3 M in magnitude.  Seeds outside, more than kSampleRow samples, no table: the engine.
constexpr uint32_t kSampleWindowHalf = 1u << 22;
constexpr uint32_t kSampleWindow = 1u << 23;
constexpr int kSampleRow = 8;

struct RenderParams {
    const uint8_t* scene;  // flat blob in HBM
    const uint32_t* seed_table;  // kSeedWindow words, or NULL: every hit seeds by the recurrence
    const uint32_t* seed_table_full;  // mt[397] for EVERY 32-bit seed (16 GiB, built on a device's first ambient-occlusion
                                      // render: the AO seeds, raytracer.cpp:122-123, cover the whole range), or NULL
    mcrt_config cfg;
    Shard shard;
    int layout;            // MCRT_LAYOUT_*
    float* out;            // float4 frame or packed rows (may be NULL when out8 is given)
    uint8_t* out8;         // RGBA8 frame or packed rows, quantised in the epilogue (may be NULL)
    uint32_t* tile_rng;    // owned_tiles x stream_parts x 624 mt19937 state words (NULL when no tile draws)
    const float4* bg_plate;  // the device's background plate of this frame configuration (below), or NULL: `plan_tiles` computes
                           //    the gradient background tiles itself
    const float* draw_plate;  // the device's draw plate of this frame configuration (below), or NULL: `plan_tiles` makes the touched
                           //    tiles' draws itself, into ws.tile_draws
    const float4* sample_table;  // the device's sample table (kSampleWindow rows, above), or NULL: every traced hit runs its engine
    WaveSpace ws;
    int draws_per_sample;  // 0, 2 or 4
    int stream_waves;      // waves per tile in `plan_tiles` (1, 2 or 4, <= stream_parts; choose_grids)
    int stream_parts;      // a tile's mt19937 stream can be generated in this many parts (1, 2 or 4),
    int stream_part_twists;  //   of this many 624-word twists each, from engine states kept with the tile seeds (tile_rng:
                           //   owned_tiles x stream_parts x 624 words)
    int parts_per_tile;    // a tile that meshes can touch is split into at most this many work units
    int unit_blocks;       // 1: the units of a tile are the blocks of a unit_gx x unit_gy grid, unit_bw x unit_bh pixels each (clipped
                           //    with the tile; choose_parts_per_tile); 0 (MCRT_UNIT_BLOCKS=0, renderTile rectangles): pixel ranges
    int unit_gx, unit_gy, unit_bw, unit_bh;
    int lds_alpha_words;   // dynamic LDS: alpha-predicate words staged per workgroup
    int lds_face_entries;  // dynamic LDS: n_meshes * 6 face-table entries
    int scene_in_lds;      // 1 when both tables fit the LDS budget (otherwise the kernels read HBM)
    int scene_posed;       // 1 when any mesh has a rotation (selects the kernels that carry the local-frame path)
    int rows_per_batch;    // owned tile rows per pipeline pass
    int bg_in_plan;        // 1: `plan_tiles` renders the background tiles from the draws in LDS and only touched tiles' draws
                           //    go to HBM; 0 (more than 24 draws per pixel): all streams to HBM, `primary` renders them
    int bg_kernel;         // 1 (bg_in_plan == 0 and many samples per pixel): `background_kernel` renders the background tiles from their
                           //    streams, slab by slab through LDS; 0: `primary`'s tail does, a lane per pixel straight from HBM
    int background;        // MCRT_BACKGROUND_*.  TRANSPARENT: background tiles are (0,0,0,0) without draws (`plan_tiles`; bg_in_plan
                           //    is then 1 and bg_kernel 0 at every sample count) and `resolve_transparent` sums the samples that hit only
    int lit_round;         // `lit`: records per round (a block of 256)
    int lit_pass;          // `lit`: traced records per pass (their light samples live in LDS between two phases)
    int lit_lds_offset;    // `lit`: byte offset of that area in dynamic LDS (behind the scene tables, 16-aligned)
    int lit_lds_bytes;     // `lit`: its size
    int flat;              // 1: flat pipeline (all levels' records shaded at once); 0: general variants, one launch set per level
    float inv_width, inv_height;  // 1.0f / width, 1.0f / height (correctly rounded: formed on the host)
    int div_frame;         // 1: width and height lie in rt::div_frame's verified range (rt_core.h)
    int inside_fast;       // shadow / AO rays: 1 — a candidate whose box holds the ray's origin strictly inside takes
                           //    rt::mesh_candidate_inside (the exit face alone); 0 (MCRT_INSIDE_FAST=0) — the general routine
    int bundle_decisions;  // `lit`: 1 — a hit whose whole bundle of shadow rays is decided (rt::bundle_decide) draws no light
                           //    samples and traces no rays; 0 (MCRT_BUNDLE_DECISIONS=0) — every hit's rays are traced
    int work_tickets;      // `primary`, `lit`: 1 — a workgroup claims the items of the work list behind its first by ticket (an atomic
                           //    counter per kernel); 0 (MCRT_WORK_TICKETS=0) — it strides over the list by the grid's size
    int shared_device;     // 1: this render shares the device with others (another lane of its frame, or another handle's frame still
                           //    running when it was enqueued): the grids below are then sized for throughput — fewer, longer-lived
                           //    workgroups per kernel leave room for the other frames' kernels —, otherwise for the frame's own latency
    int grid_primary, grid_ao, grid_lit, grid_resolve;  // workgroup caps of the launches (choose_grids; all kernels stride)
    int rect_x, rect_y, rect_w, rect_h;  // rect_w > 0: the launch renders ONE tile, this rectangle (TileRenderer::renderTile for an
                           //    arbitrary Tile, tile_renderer.cpp:71-127: seed rect_y * width + rect_x, pixels in the rectangle's own
                           //    row-major order); the shard is then one tile row of one tile
};

// ---- extra lights (include/mcrt.h, "extra lights"): the handle's lights 1 .. n_extra; light 0 is the scene header's.  They
// travel as an argument of their own to the kernels that read them (render_kernels.hip, "extra lights") and are no part of
// RenderParams: a larger RenderParams would move the arguments of every kernel that was there before.
constexpr int kMaxLights = MCRT_MAX_EXTRA_LIGHTS + 1;
struct LightSet {
    int n_extra;
    int reserved[3];
    mcrt_light_source extra[MCRT_MAX_EXTRA_LIGHTS];
};

// ======== planning (render_plan.cpp): pure host code ========
Shard make_shard(const mcrt_config& cfg, int first, int step);
inline int owned_tiles(const RenderParams& p) { return p.shard.owned_rows * p.shard.tiles_x; }
inline bool soft_sampling(const mcrt_config& c) { return c.soft_shadows && c.shadow_samples > 1; }

// Whether a scene's tables fit the LDS budget, the sizes a kernel then stages (0 / 0 when it reads them from HBM) and the
// kernel variant the scene needs (launch_shapes.h: kViewHbm, kViewLds or kViewLdsUnposed).  One rule for the beauty path
// and the layers and ground passes.
constexpr int kAlphaLdsWordsMax = 4096;  // 64 Ki texels
constexpr int kFaceLdsEntriesMax = 384;   // 64 meshes
struct LdsFit { int face_entries, alpha_words, view; };
LdsFit lds_fit(uint32_t alpha_words, uint32_t n_meshes, bool posed);
// A pass's frame record (LayersFrame, GroundFrame, ... BakeFrame): fills f.lds_* for a scene of that size and returns the
// kernel variant it needs
template <class Frame>
int view_of_frame(Frame& f, uint32_t alpha_words, uint32_t n_meshes, bool posed) {
    const LdsFit fit = lds_fit(alpha_words, n_meshes, posed);
    f.lds_alpha_words = fit.alpha_words, f.lds_face_entries = fit.face_entries;
    return fit.view;
}
// the variant of a batch of such frames: the most general any of them needs; rewrites the frames' LDS fields where it reads HBM
template <class Frame>
int batch_view_of(Frame* frames, const int* views, int n) {
    bool any_hbm = false, any_posed = false;
    for (int i = 0; i < n; ++i) {
        any_hbm = any_hbm || views[i] == kViewHbm;
        any_posed = any_posed || views[i] == kViewLds;
    }
    if (any_hbm)
        for (int i = 0; i < n; ++i) frames[i].lds_alpha_words = 0, frames[i].lds_face_entries = 0;
    return any_hbm ? kViewHbm : (any_posed ? kViewLds : kViewLdsUnposed);
}
// dynamic LDS of the scene tables p's kernels stage
inline size_t scene_table_bytes(const RenderParams& p) { return p.scene_in_lds ? scene_tables_lds_bytes(p.lds_face_entries, p.lds_alpha_words) : 0; }

// Sizes of the workspace arrays for p.cfg / p.shard; fills p.parts_per_tile, p.rows_per_batch and
// p.ws.cap / p.ws.stack_stride.  budget_bytes bounds the per-batch workspace (a batch is never
// smaller than one tile row).
struct WorkspaceBytes {
    size_t tile_rng, tile_draws, scol, end, units, unit_hits, tile_mask, queue_each, texel_refs, targets, cand, lit0, lit1, stack, counters, hit_rng;
};
// row_touched[j]: upper bound of the tiles meshes can touch in owned tile row j (NULL: every tile).
// extra_lights > 0: the general variants, with `targets`, `cand` and `lit` sized for extra_lights + 1 lights per record.
WorkspaceBytes plan_workspace(RenderParams& p, size_t budget_bytes, const int* row_touched, int extra_lights = 0);
// fills p.shared_device, p.grid_* and p.stream_waves (MCRT_*_GRID / MCRT_STREAM_WAVES override, development knobs)
void choose_grids(RenderParams& p, bool shared_device, bool company);  // company: other frames or lanes run beside this launch set
constexpr int kCounterWords = 4096;

// ---- background plate: the finished pixels of every gradient background tile of a frame configuration.  Such a tile's
// pixels are a function of the frame's size, the tile size, the samples per pixel, the draws per sample, the gradient's
// settings and the div_frame mode alone (the jitter comes from the tile's own mt19937 stream, seeded tile.y * width + tile.x);
// scene, camera, light, shard and output layout do not enter.  Tile-major over ALL tiles of the frame: global tile
// ty * tiles_x + tx owns tile_size^2 float4, a clipped edge tile's w x h pixels row-major at the front of its slot.  The
// slots of the one-colour tiles (constant_background) are never written and never read.  Built once per device and key by
// launch_fill_bg_plate with the code `plan_tiles` runs without a plate, immutable afterwards: `plan_tiles` copies from it.

// whether a frame prepared as `p` can take a plate: opaque gradient background, jittered samples, rendered in `plan_tiles`,
// a whole-frame entry point (not a renderTile rectangle)
bool bg_plate_eligible(const RenderParams& p);
// bytes of the plate of cfg's frame; 0 when the size does not fit 32-bit pixel indices
size_t bg_plate_bytes(const mcrt_config& cfg);
// bytes of the scratch launch_fill_bg_plate needs: the engine states of every tile of the frame
size_t bg_plate_rng_bytes(const RenderParams& p);
// p with the whole-frame shard and no outputs: the parameters the plates' fill launches and their scratch sizes take
RenderParams bg_plate_fill_params(const RenderParams& p);

// ---- draw plate: the mt19937 draws of EVERY tile of a frame configuration, as uniform floats — what `plan_tiles` writes
// into a touched tile's slot of ws.tile_draws.  A tile's draws are a function of the frame's size, the tile size, the
// samples per pixel and the draws per sample alone (the engine is seeded tile.y * width + tile.x): scene, pose, camera,
// light, bounces, background, shard, layout and lanes do not enter.  [frame tile index (TileGeom::frame_tile)][draws_stride]
// floats, a clipped tile's shorter stream at the front of its slot.  Built once per device and key by
// launch_fill_draw_plate with the routine `plan_tiles` runs (tile_stream_wave), immutable afterwards: with a plate
// `plan_tiles` twists nothing for a touched tile, and `primary` and `resolve` read the tile's draws from the plate.

// whether a frame prepared as `p` can take a draw plate: jitter or lens draws, the touched-tiles layout (bg_in_plan), at
// most 24 draws per pixel (the streams of 64 spp frames are gigabytes), a whole-frame entry point
bool draw_plate_eligible(const RenderParams& p);
// bytes of the plate of p's frame (p.ws.draws_stride set: plan_workspace); 0 when the frame cannot have one
size_t draw_plate_bytes(const RenderParams& p);
// bytes of the scratch launch_fill_draw_plate needs: the engine states of every tile of the frame
size_t draw_plate_rng_bytes(const RenderParams& p);

// ---- batches (mcrt_render_batch_device): N frames of one config in ONE launch sequence, blockIdx.y = frame; each
// frame's RenderParams (its own scene, workspace, counters and output) are read from a device-resident table
// whether the batched kernels can take a frame: flat pipeline, a whole-frame shard, one pass (rows_per_batch >= owned rows)
bool batch_eligible(const RenderParams& p);
// frames of one launch sequence share the background mode (it selects the `resolve` kernel)
struct BatchPlan {
    int view = 0;        // the kernel variant of the whole batch (the most general any frame needs)
    size_t dyn = 0;      // dynamic LDS of primary / ao: the largest frame's scene tables
    size_t lit_dyn = 0;  // dynamic LDS of lit: the largest frame's lit_lds_offset + lit_lds_bytes
};
constexpr int kBatchMaxFrames = 256;  // frames per launch sequence (larger batches are split: render_plan.cpp, batch_grid)
// Makes frames[0..n) one batch: picks the variant (rewriting the frames' LDS fields where it reads HBM), checks the
// lit_lds_offset invariant per frame and sets the grids (choose_grids with company, then the batch rule).
// hipErrorInvalidValue when a frame is not eligible or the frames do not share the config's launch shapes.
hipError_t plan_batch(RenderParams* frames, int n, bool others_running, BatchPlan& plan);

// ---- geometry layers (mcrt_render_layers_device & co): what is under each pixel — one pixel-centre ray per pixel
// (Camera::generateRay at u = (px + 0.5f) / width, v = (py + 0.5f) / height), intersectScene, no draws, no shading.  The pass
// reads the scene blob alone: no workspace, no counters.
// One frame of a layers pass: its scene and its planes (any may be NULL, not all), row-major, width * height pixels each
struct LayersFrame {
    const uint8_t* scene;
    float* depth;          // 1 float per pixel: HitResult::t, FLT_MAX at a miss
    float4* normal;        // HitResult::normal, w = 0; zero at a miss
    float4* albedo;        // HitResult::textureColor; zero at a miss
    int4* id;              // {mesh, face slot | MCRT_ID_BACK | MCRT_ID_OUTER, tx, ty}; {-1, 0, -1, -1} at a miss
    int lds_alpha_words;   // scene tables staged in LDS (as RenderParams'), 0 / 0 when the kernel reads them from HBM
    int lds_face_entries;
};
// what the frames of one launch share: the frame's size (cfg: only width, height and tile_size are read) and its tile grid
struct LayersShape {
    mcrt_config cfg;
    int tiles_x, tiles_y;
    int parts;  // work units per tile: a workgroup takes 256 pixels of a tile
};
// false when the frame holds more units than the kernels index (2^31)
bool make_layers_shape(const mcrt_config& cfg, LayersShape& shape);
constexpr int kLayersBatchMaxFrames = 4096;  // frames per launch (blockIdx.y; larger batches take several launches)
size_t layers_lds_bytes(const LayersFrame& f);

// ---- ground shadow (mcrt_render_ground_device & co): the figure's shadow on the plane y = ground_y — per pixel the
// pixel-centre ray of the layers, its point P on the plane, and computeSoftShadow(P, (0, 1, 0)) with the seed the reference
// forms for a hit at depth 0.  Like a layers pass it reads the scene blob alone (and the device's seed table).
// One frame of a ground pass: its scene, its height and its planes (any may be NULL, not all), width * height pixels each
struct GroundFrame {
    const uint8_t* scene;
    float* visibility;           // 1 float per pixel: lit light samples / samples; 1.0f where the ray misses the plane
    float* distance;             // the ray parameter t of the plane; FLT_MAX where the ray misses it
    uint8_t* matte;              // quantised 1 - visibility: the alpha of a black shadow image
    const uint32_t* seed_table;  // the handle's window table (RenderParams::seed_table), or NULL: the recurrence
    float ground_y;
    int lds_alpha_words;         // scene tables staged in LDS, as LayersFrame's
    int lds_face_entries;
};
constexpr int kGroundMaxSamples = 113;  // the truncated engine's 227 draws: no per-lane 624-word state
// what the frames of one launch share
struct GroundShape {
    LayersShape tiles;     // the frame's size and its tile grid, as a layers pass cuts it
    int samples;           // S: shadow_samples when soft_shadows && shadow_samples > 1, else 1
    int pass;              // undecided pixels whose S sample positions fit the block's LDS area at once
    int bundle_decisions;  // as RenderParams'
    int inside_fast;
};
// false when the frame holds more units than the kernels index (2^31)
bool make_ground_shape(const mcrt_config& cfg, bool bundle_decisions, bool inside_fast, GroundShape& shape);
// dynamic LDS of a launch: the frame's scene tables, then the block's area (masks, points, counts and sample positions)
size_t ground_lds_bytes(const GroundFrame& f, const GroundShape& shape);

// ---- ground occlusion (mcrt_render_ground_occlusion_device & co): the figure's contact occlusion on the plane y = ground_y — per
// pixel the ground pass's ray and point P, and computeAO(P, (0, 1, 0)) with the seed the reference forms for a hit at P.  Reads
// the scene blob and, where the handle holds it, the device's table of all seeds.
// One frame of a ground-occlusion pass: its scene, its height and its planes (either may be NULL, not both)
struct GroundOcclusionFrame {
    const uint8_t* scene;
    float* occlusion;                 // 1 float per pixel: 1 - occluded / ao_samples; 1.0f where the ray misses the plane
    uint8_t* matte;                   // quantised 1 - occlusion: the alpha of a black contact-shadow image
    const uint32_t* seed_table_full;  // the device's table of all seeds where a render has built it, or NULL: the recurrence
    float ground_y;
    int lds_alpha_words;              // scene tables staged in LDS, as LayersFrame's
    int lds_face_entries;
};
// what the frames of one launch share
struct GroundOcclusionShape {
    LayersShape tiles;  // the frame's size and its tile grid, as a layers pass cuts it
    int ao_samples;     // A: 1 .. kLightMaxSamples
    float ao_radius;    // <= 0: nothing is traced
    int pass;           // traced pixels whose A directions fit the block's LDS area at once
    int inside_fast;    // as RenderParams'
};
// false when the frame holds more units than the kernels index (2^31)
bool make_ground_occlusion_shape(const mcrt_config& cfg, bool inside_fast, GroundOcclusionShape& shape);
// dynamic LDS of a launch: the frame's scene tables, then the block's area (masks, points, counts, the traced list and directions)
size_t ground_occlusion_lds_bytes(const GroundOcclusionFrame& f, const GroundOcclusionShape& shape);

// ---- ground reflection (mcrt_render_reflection_device & co): the figure mirrored in the plane y = ground_y — per pixel the
// pixel-centre ray of the layers, its point P on the plane, the reference's reflection ray for a hit at P with normal (0, 1, 0),
// and traceRay(that ray, depth 1): shading, shadows and further bounces as the reference's recursion runs them below a depth-0
// surface.  Reads the scene blob and the device's seed table, like a ground pass.
// One frame of a reflection pass: its scene, its height and its planes (any may be NULL, not all), width * height pixels each
struct ReflectionFrame {
    const uint8_t* scene;
    float* rgba;                 // 4 floats per pixel, straight alpha; zero where the plane is not reached or the reflected ray misses
    uint8_t* rgba8;              // the same colour quantised as mcrt_quantize_rgba8 quantises it
    float* distance;             // HitResult::t of the reflection ray's closest hit; FLT_MAX without one
    const uint32_t* seed_table;  // the handle's window table, or NULL: the recurrence
    float ground_y;
    int lds_alpha_words;         // scene tables staged in LDS, as LayersFrame's
    int lds_face_entries;
};
constexpr int kReflectMaxBounces = 8;  // levels of the per-lane colour stack (the depth the flat pipeline is laid out for: kFlatMaxBounces)
// what the frames of one launch share
struct ReflectionShape {
    LayersShape tiles;     // the frame's size and its tile grid, as a layers pass cuts it
    int samples;           // S: shadow_samples when soft_shadows && shadow_samples > 1, else 1
    int pass;              // undecided hits whose S sample positions fit the block's LDS area at once
    int max_bounces;       // below 1: every pixel keeps the miss constants
    int bundle_decisions;  // as RenderParams'
    int inside_fast;
    int cull;              // 0 (MCRT_REFLECT_CULL=0): every mesh is tested for every tile
};
// false when the frame holds more units than the kernels index (2^31)
bool make_reflection_shape(const mcrt_config& cfg, bool bundle_decisions, bool inside_fast, bool cull, ReflectionShape& shape);
// dynamic LDS of a launch: the frame's scene tables, then the block's area (hit records, masks, counts and sample positions)
size_t reflection_lds_bytes(const ReflectionFrame& f, const ReflectionShape& shape);

// ---- light layers (mcrt_render_light_device & co): what the light does at the geometry layers' primary hit — the visibility
// term of shade() (computeSoftShadow with the depth-0 seed, or shade()'s own isInShadow test), computeAO, and shade() with that
// visibility.  Reads the scene blob and the device's seed tables, like a ground pass.
// One frame of a light pass: its scene and its planes (any may be NULL, not all), width * height pixels each
struct ShadeFrame {
    const uint8_t* scene;
    float* visibility;                // 1 float per pixel: the shadow factor of the hit; 1.0f at a miss
    float* occlusion;                 // 1 float per pixel: computeAO; 1.0f at a miss
    float* direct;                    // 4 floats per pixel: shade() with that visibility, alpha = the texel's; zero at a miss
    const uint32_t* seed_table;       // the handle's window table (RenderParams::seed_table), or NULL: the recurrence
    const uint32_t* seed_table_full;  // the device's table of all seeds where a render has built it, or NULL: the recurrence
    int lds_alpha_words;              // scene tables staged in LDS, as LayersFrame's
    int lds_face_entries;
};
constexpr int kLightMaxSamples = 113;  // shadow and AO samples: the truncated engine's 227 draws, two per sample
// what the frames of one launch share
struct ShadeShape {
    LayersShape tiles;     // the frame's size and its tile grid, as a layers pass cuts it
    int samples;           // S: shadow_samples when soft_shadows && shadow_samples > 1, else 1
    int pass;              // undecided hits whose S sample positions fit the block's LDS area at once
    int ao_samples;        // A (read by `occlusion` alone)
    float ao_radius;
    int bundle_decisions;  // as RenderParams'
    int inside_fast;
};
// false when the frame holds more units than the kernels index (2^31)
bool make_shade_shape(const mcrt_config& cfg, bool bundle_decisions, bool inside_fast, ShadeShape& shape);
// dynamic LDS of the two launches: the frame's scene tables, then the block's area
size_t shade_lds_bytes(const ShadeFrame& f, const ShadeShape& shape);  // hit records, masks, counts and sample positions
size_t occlusion_lds_bytes(const ShadeFrame& f);                         // hit records, masks, the traced list and the values

// ---- light bake (mcrt_bake_light_device & co): the light layers' terms per TEXEL of the scene's pool, at points of the texel on
// its owner face (include/mcrt.h, "light bake") — no camera, no tiles.  Reads the scene blob, the handle's owner-face list and
// the device's seed tables.
// One owner face: the pool texels tex_off .. tex_off + w * h - 1 are baked on face `code & 7` of mesh `code >> 3`
struct BakeFace {
    int32_t tex_off, w, h, code;
};
// The owner faces of the flattened scene `blob` (header and mesh table are read), sorted by tex_off: of the faces that share a
// texture the one with the lowest mesh index, then the lowest face slot.  Their ranges are disjoint (flatten.cpp gives every
// texture a range of its own).
void bake_owner_faces(const uint8_t* blob, std::vector<BakeFace>& out);
// One frame of a bake: its scene, its owner faces and its planes (any may be NULL, not all), n_texels texels each
struct BakeFrame {
    const uint8_t* scene;
    const BakeFace* faces;            // device memory, behind the handle's blob
    int n_faces, n_texels;
    float4* position;                 // the texel centre's P, w = 1 live / 0 dead; zero without an owner
    float4* normal;                   // N, w = 0; zero without an owner
    float* visibility;                // mean of the sub-samples' shadow factors; 1.0f for a dead texel
    float* occlusion;                 // mean of computeAO; 1.0f for a dead texel
    float* direct;                    // 4 floats per texel: mean of shade(); zero for a dead texel
    const uint32_t* seed_table;       // as ShadeFrame's
    const uint32_t* seed_table_full;
    int lds_alpha_words;              // scene tables staged in LDS, as LayersFrame's
    int lds_face_entries;
};
constexpr int kBakeMaxGrid = 4;
// what the frames of one launch share
struct BakeShape {
    int grid;              // q: q * q sub-samples per texel
    int samples;           // S: shadow_samples when soft_shadows && shadow_samples > 1, else 1
    int pass;              // undecided points whose S sample positions fit the block's LDS area at once
    int ao_samples;        // A (read by `bake_occlusion` alone)
    float ao_radius;
    int bundle_decisions;  // as RenderParams'
    int inside_fast;
    int max_units;         // work units (256 pool texels) of the largest frame
    int geometry;          // set per launch: this kernel writes the position and normal planes
    int rays;              // `bake_shade`: visibility or direct is asked for (otherwise it writes position / normal alone)
};
void make_bake_shape(const mcrt_config& cfg, int grid, bool bundle_decisions, bool inside_fast, int max_texels, BakeShape& shape);
// dynamic LDS of the two launches: the frame's scene tables, then the block's area
size_t bake_shade_lds_bytes(const BakeFrame& f, const BakeShape& shape);  // point records, texel records, masks, counts and sample positions
size_t bake_occlusion_lds_bytes(const BakeFrame& f);                         // point records, texel records, masks, the traced list and the values

// ---- light layers and bake under extra lights (mcrt_render_light_multi_device, mcrt_bake_light_multi_device & co; include/mcrt.h,
// "light layers and bake under extra lights"): one visibility and one direct plane per light — light 0 the scene's own, lights
// 1 .. n_extra the handle's, read BY VALUE at enqueue — and their clamped sum.  Kernels of their own (`shade_lights`,
// `bake_shade_lights`) over frame records of their own, which carry the lights so that the table of a batch gives every frame
// its own; ShadeShape / BakeShape, the LDS areas and their size functions are the single-light kernels'.  The occlusion plane
// does not read a light: it is the `occlusion` / `bake_occlusion` kernels' over a ShadeFrame / BakeFrame with that plane alone.
// Of the base record `visibility`, `occlusion` and `direct` stay NULL; a bake's `position` and `normal` are the base's.
struct ShadeLightsFrame : ShadeFrame {
    LightSet lights;
    float* vis[kMaxLights];     // 1 float per pixel: light k's shadow factor; a light the handle lacks: the miss constant 1.0f
    float* dir[kMaxLights];     // 4 floats per pixel: shade() for light k alone (k >= 1: ambient 0); a light the handle lacks: zero
    float* combined;            // 4 floats per pixel: clamp(D_0 + D_1 + ..), alpha D_0's
};
struct BakeLightsFrame : BakeFrame {
    LightSet lights;
    float* vis[kMaxLights];     // the means of the sub-samples' values, per texel
    float* dir[kMaxLights];
    float* combined;            // the mean of the sub-samples' clamped sums
};
inline bool any_light_plane(float* const (&vis)[kMaxLights], float* const (&dir)[kMaxLights], const float* combined) {
    bool any = combined != nullptr;
    for (int k = 0; k < kMaxLights; ++k) any = any || vis[k] || dir[k];
    return any;
}

// ---- skins on resident scenes (mcrt_scene_set_skin_device & co): a repaintable handle's blob holds the full mesh table of
// its skin kind, so texel i of its pool is cut from one fixed pixel of the skin image.  One workgroup per scene rewrites what
// a skin decides of the blob: the float4 texel pool (u8 / 255.0f through a table the HOST formed), the 2-bit alpha predicates
// and the MESH_OPAQUE bit of every mesh.  Nothing else of the blob is touched.
constexpr int kSkinMaxMeshes = 12;
constexpr int kSkinMaxTexels = 3264;
// what the scenes of one launch share.  `tables` (device_stores.cpp, per device and skin kind): 256 floats i / 255.0f, then
// n_texels uint16 (mesh << 12) | skin pixel index y * 64 + x, in pool order.
struct SkinPaintShape {
    const void* tables;
    int n_texels;        // 3264 (64x64), 3136 (64x64 slim) or 2016 (64x32)
    int n_meshes;        // 12 or 7
    int skin_bytes;      // 64 * height * 4
    uint32_t mesh_offset, texel_offset, alpha_offset, alpha_words;  // of the kind's blob (FlatHeader)
};
constexpr int kSkinBatchShapes = 2;  // the shapes one batch launch carries: the two 64x64 models may be mixed in it
struct SkinPaintFrame {
    uint8_t* scene;       // the resident blob
    const uint8_t* skin;  // RGBA8, row-major, 4-byte aligned
    int kind;             // a batch launch: which of its kSkinBatchShapes shapes this frame takes (0 or 1); else 0
    int reserved[3];      // (32 bytes: a frame is two aligned scalar loads)
};
size_t skin_tables_bytes(int n_texels);

// ---- capes on resident scenes (mcrt_scene_set_cape_device & co): a caped handle's blob holds the cape as its LAST mesh, its
// 372 texels behind the skin's in the pool.  The skin's texel counts are all multiples of 16, so the cape's 24 alpha-predicate
// words are its own.  One workgroup per scene rewrites what a cape image decides of the blob: those texels, those words and the
// cape mesh's MESH_OPAQUE bit.  Nothing else of the blob is touched — the skin kernels above, given the skin's counts and
// n_meshes without the cape, in turn leave the cape's alone.
constexpr int kCapeTexels = 372;       // faces 10x16, 10x16, 1x16, 1x16, 10x1, 10x1
constexpr int kCapeImageBytes = 64 * 32 * 4;
constexpr int kCapeAlphaWords = 24;    // the last one holds 4 texels
constexpr int kCapedMaxMeshes = kSkinMaxMeshes + 1;
// what the scenes of one launch share.  `tables` (device_stores.cpp, per device): 256 floats i / 255.0f, then kCapeTexels
// uint16 cape pixel indices y * 64 + x, in pool order.
struct CapePaintShape {
    const void* tables;
};
// Where the cape lies travels with the frame, not the shape: a slim skin's pool is shorter than a classic one's, and the two
// models mix in one launch.  Read through the frame table these are scalar loads like the pointers.
struct CapePaintFrame {
    uint8_t* scene;         // the resident blob
    const uint8_t* cape;    // 64x32 RGBA8, row-major, 4-byte aligned; NULL: a transparent cape
    uint32_t flags_offset;  // of the cape mesh's FlatMesh::flags in the blob
    uint32_t texel_offset;  // of the cape's first texel, a multiple of 16
    uint32_t alpha_offset;  // of the cape's first alpha-predicate word
    uint32_t reserved;      // (32 bytes: a frame is two aligned scalar loads)
};
size_t cape_tables_bytes();

// ---- views of resident scenes (mcrt_scene_set_view_device & co): the prefix [FlatHeader][FlatMesh x n] of a repaintable
// handle's blob is what pose, camera and light decide, but for the MESH_OPAQUE bit of every FlatMesh::flags, which the skin
// owns.  One wave per scene copies a table the host flattened (flatten_view_table) over that prefix in 16-byte chunks and
// keeps those bits as the blob has them.  Nothing from texel_offset on is touched.
constexpr int kViewMaxChunks = 192;  // 64 lanes x 3 chunks: (192 + 12 * 192) / 16 = 156 for a 64x64 skin, 96 for a 64x32 one; with a cape mesh 168 and 108
struct SceneViewShape {
    uint32_t mesh_offset;  // of the kind's blob (FlatHeader), a multiple of 16
    int n_meshes;          // 12 or 7; 13 or 8 for a caped handle (168 or 108 chunks)
    int n_chunks;          // texel_offset / 16
};
struct SceneViewFrame {
    uint8_t* scene;        // the resident blob
    const uint8_t* table;  // the staged prefix in device memory, 16-byte aligned
};

// ---- studio shot (mcrt_composite_shot_batch_device & co): the blend of include/mcrt.h — the straight-alpha figure over a page
// with the ground shadow and the floor reflection — per pixel, from planes that are already on the device.  Of the scene it
// reads the header's background colour alone, and only for MCRT_PAGE_REFERENCE without a gradient.
// One frame of a shot: its inputs (all but the figure may be NULL) and its outputs (either may be NULL, not both)
struct ShotFrame {
    const uint8_t* scene;
    const float* figure;      // 4 floats per pixel: the MCRT_BACKGROUND_TRANSPARENT frame, straight alpha
    const float* visibility;  // 1 float per pixel: the ground pass's; NULL: 1.0f everywhere
    const float* reflection;  // 4 floats per pixel: the reflection pass's rgba; NULL: (0, 0, 0, 0) everywhere
    const float* distance;    // 1 float per pixel: the reflection pass's; read only with reflection_fade > 0
    const float* occlusion;   // 1 float per pixel: the ground-occlusion pass's; NULL: 1.0f everywhere
    float* out;               // 4 floats per pixel
    uint8_t* out8;            // RGBA8, quantised as mcrt_quantize_rgba8 quantises it
};
// what the frames of one launch share: the frame's size and gradient (cfg) and the shot's settings
struct ShotShape {
    mcrt_config cfg;
    int page;  // MCRT_PAGE_*; MCRT_PAGE_TRANSPARENT from the _ex entries alone
    float page_color[3];
    float shadow_strength, reflectivity, reflection_fade;
    float floor_occlusion;  // o, 0..1: read only where a frame has an occlusion plane
    float shadow_color[3];  // C: (0, 0, 0) from the plain and _occ entries
};

// ======== pipeline launches (render_kernels.hip) ========
// seeds p.tile_rng: one mt19937 per owned tile (tile_renderer.cpp:78).  A function of the frame width, the
// tile size and the shard only — the caller keeps the result across renders and calls this when those change.
hipError_t launch_seed_tiles(const RenderParams& p, hipStream_t stream);
// enqueue the whole pipeline of one lane on `stream` (p.tile_rng already seeded): per batch of tile rows
// plan → primary (+ the primary hits' reflection rays) → (ao →) lit (the rest of the chains, then light and shade) → resolve
// Optional events for a caller that downloads tile rows as they become final (the one-shot host path):
//  after_plan    recorded behind the first pass's plan_tiles: with bg_in_plan every tile row that holds no touched
//                tile is complete then
//  batch_done[b] recorded behind pass b's resolve: the rows of that pass are complete (n_batch_done entries, may be 0)
struct LaunchMarks {
    hipEvent_t after_plan = nullptr;
    hipEvent_t* batch_done = nullptr;
    int n_batch_done = 0;
};
// lights with n_extra > 0 (p planned for them: plan_workspace): the levels run the multi-light stages
hipError_t launch_render(const RenderParams& p, hipStream_t stream, const LaunchMarks* marks = nullptr, const LightSet* lights = nullptr);
// Fills `plate` for p's configuration (p: any eligible frame's parameters; its shard, layout and outputs are not read).
// `tile_rng` is scratch of bg_plate_rng_bytes(p) bytes.  Enqueues on `stream`; the caller synchronises.
hipError_t launch_fill_bg_plate(const RenderParams& p, float4* plate, uint32_t* tile_rng, hipStream_t stream);
// Fills `plate` for p's configuration (p: any eligible frame's parameters; its shard, layout and outputs are not read).
// `tile_rng` is scratch of draw_plate_rng_bytes(p) bytes.  Enqueues on `stream`; the caller synchronises.
hipError_t launch_fill_draw_plate(const RenderParams& p, float* plate, uint32_t* tile_rng, hipStream_t stream);
// seeds the tile streams of the frames in d_table (launch_seed_tiles for each); p0: any one of them (host copy)
hipError_t launch_seed_tiles_batch(const RenderParams& p0, const RenderParams* d_table, int n_frames, hipStream_t stream);
// plan → (background) → primary → (ao) → lit → resolve, one launch each for all n_frames (<= kBatchMaxFrames) frames
hipError_t launch_render_batch(const RenderParams& p0, const BatchPlan& plan, const RenderParams* d_table, int n_frames, hipStream_t stream);

// ======== passes (pass_kernels.hip): layers and picks, ground shadow, ground occlusion, ground reflection, light layers, light bake, studio shot, skin repaints, cape repaints, views ========
hipError_t launch_layers(const LayersFrame& f, const LayersShape& shape, int view, hipStream_t stream);
// frames d_table[0..n_frames) (device memory, n_frames <= kLayersBatchMaxFrames), blockIdx.y = frame; max_dyn: the largest
// frame's LDS tables
hipError_t launch_layers_batch(const LayersFrame* d_table, int n_frames, const LayersShape& shape, int view, size_t max_dyn, hipStream_t stream);
// n pixels (d_xy: n x {x, y}, inside the frame) → n mcrt_surface records, by the device functions of the layers kernels
hipError_t launch_pick(const uint8_t* scene, const LayersShape& shape, const int32_t* d_xy, int n, mcrt_surface* d_out, hipStream_t stream);
hipError_t launch_ground(const GroundFrame& f, const GroundShape& shape, int view, hipStream_t stream);
// frames d_table[0..n_frames) (device memory, n_frames <= kLayersBatchMaxFrames), blockIdx.y = frame; max_dyn: the largest
// frame's ground_lds_bytes
hipError_t launch_ground_batch(const GroundFrame* d_table, int n_frames, const GroundShape& shape, int view, size_t max_dyn, hipStream_t stream);
hipError_t launch_ground_occlusion(const GroundOcclusionFrame& f, const GroundOcclusionShape& shape, int view, hipStream_t stream);
// frames d_table[0..n_frames) (device memory, n_frames <= kLayersBatchMaxFrames), blockIdx.y = frame; max_dyn: the largest
// frame's ground_occlusion_lds_bytes
hipError_t launch_ground_occlusion_batch(const GroundOcclusionFrame* d_table, int n_frames, const GroundOcclusionShape& shape, int view, size_t max_dyn,
                                         hipStream_t stream);
hipError_t launch_reflection(const ReflectionFrame& f, const ReflectionShape& shape, int view, hipStream_t stream);
// frames d_table[0..n_frames) (device memory, n_frames <= kLayersBatchMaxFrames), blockIdx.y = frame; max_dyn: the largest
// frame's reflection_lds_bytes
hipError_t launch_reflection_batch(const ReflectionFrame* d_table, int n_frames, const ReflectionShape& shape, int view, size_t max_dyn, hipStream_t stream);
// `shade` where f.visibility or f.direct, then `occlusion` where f.occlusion
hipError_t launch_light(const ShadeFrame& f, const ShadeShape& shape, int view, hipStream_t stream);
// frames d_table[0..n_frames) (device memory, n_frames <= kLayersBatchMaxFrames), blockIdx.y = frame; which kernels run (the
// frames of a call share their planes) and the largest frame's shade_lds_bytes / occlusion_lds_bytes
hipError_t launch_light_batch(const ShadeFrame* d_table, int n_frames, const ShadeShape& shape, int view, bool shade, size_t shade_dyn, bool occlusion,
                              size_t occlusion_dyn, hipStream_t stream);
// `bake_shade` where visibility, direct or no occlusion plane is asked for, then `bake_occlusion` where f.occlusion; position and
// normal are written by the first kernel that runs
hipError_t launch_bake(const BakeFrame& f, const BakeShape& shape, int view, hipStream_t stream);
// frames d_table[0..n_frames) (device memory, n_frames <= kLayersBatchMaxFrames), blockIdx.y = frame; which kernels run (the
// frames of a call share their planes) and the largest frame's bake_shade_lds_bytes / bake_occlusion_lds_bytes
hipError_t launch_bake_batch(const BakeFrame* d_table, int n_frames, const BakeShape& shape, int view, bool shade, size_t shade_dyn, bool occlusion,
                             size_t occlusion_dyn, hipStream_t stream);
// `shade_lights` / `bake_shade_lights` alone (the occlusion plane of the multi-light entries goes through launch_light /
// launch_bake over a record of its own); dyn: shade_lds_bytes / bake_shade_lds_bytes of the frame, of the largest frame in a batch.
// A bake's kernel writes position and normal too (BakeShape::geometry and ::rays are set here).
hipError_t launch_light_multi(const ShadeLightsFrame& f, const ShadeShape& shape, int view, hipStream_t stream);
hipError_t launch_light_multi_batch(const ShadeLightsFrame* d_table, int n_frames, const ShadeShape& shape, int view, size_t max_dyn, hipStream_t stream);
hipError_t launch_bake_multi(const BakeLightsFrame& f, const BakeShape& shape, int view, hipStream_t stream);
hipError_t launch_bake_multi_batch(const BakeLightsFrame* d_table, int n_frames, const BakeShape& shape, int view, size_t max_dyn, hipStream_t stream);
// The blend of every shot entry (include/mcrt.h, "studio shot" and "cut-out").  d_bounds: NULL, or 4 int32 per frame of the launch
// (frame blockIdx.y at d_bounds + 4 * blockIdx.y) that already hold {width, height, 0, 0} in stream order
// (launch_shot_bounds_init) — only with the transparent page.
hipError_t launch_shot(const ShotFrame& f, const ShotShape& shape, int32_t* d_bounds, hipStream_t stream);
// frames d_table[0..n_frames) (device memory, n_frames <= kLayersBatchMaxFrames), blockIdx.y = frame
hipError_t launch_shot_batch(const ShotFrame* d_table, int n_frames, const ShotShape& shape, int32_t* d_bounds, hipStream_t stream);
// {width, height, 0, 0} into each of the n entries of d_bounds
hipError_t launch_shot_bounds_init(int32_t* d_bounds, int n, int width, int height, hipStream_t stream);
hipError_t launch_skin_paint(const SkinPaintFrame& f, const SkinPaintShape& shape, hipStream_t stream);
// frames d_table[0..n_frames) (device memory, n_frames <= kLayersBatchMaxFrames), blockIdx.y = frame; frame i takes
// shapes[frame i's kind] — the two 64x64 models of one batch; a batch of one kind passes its shape twice
hipError_t launch_skin_paint_batch(const SkinPaintFrame* d_table, int n_frames, const SkinPaintShape shapes[kSkinBatchShapes], hipStream_t stream);
bool cape_frame_ok(const CapePaintFrame& f);  // alignment and order of a frame's offsets: what the kernel's stores need
hipError_t launch_cape_paint(const CapePaintFrame& f, const CapePaintShape& shape, hipStream_t stream);
// frames d_table[0..n_frames) (device memory, n_frames <= kLayersBatchMaxFrames), blockIdx.y = frame
hipError_t launch_cape_paint_batch(const CapePaintFrame* d_table, int n_frames, const CapePaintShape& shape, hipStream_t stream);
hipError_t launch_scene_view(const SceneViewFrame& f, const SceneViewShape& shape, hipStream_t stream);
// frames d_table[0..n_frames) (device memory, n_frames <= kLayersBatchMaxFrames), blockIdx.y = frame
hipError_t launch_scene_view_batch(const SceneViewFrame* d_table, int n_frames, const SceneViewShape& shape, hipStream_t stream);

// ======== utilities and probes (util_kernels.hip) ========
hipError_t launch_unpack_rows(const mcrt_config& cfg, const Shard& sh, const float* packed, float* frame,
                              hipStream_t stream);
hipError_t launch_unpack_rows8(const mcrt_config& cfg, const Shard& sh, const uint8_t* packed, uint8_t* frame, hipStream_t stream);  // RGBA8 plane
hipError_t launch_assemble_frame(const mcrt_config& cfg, int world, const float* gathered, size_t rank_stride_pixels,
                                 float* frame, hipStream_t stream);
hipError_t launch_quantize(const float* rgba, uint8_t* out, size_t n_pixels, hipStream_t stream);
// fills table[i] = mt[397] of std::mt19937(i - kSeedWindowHalf) for i < kSeedWindow
hipError_t launch_build_seed_table(uint32_t* table, hipStream_t stream);
// fills table[s] = mt[397] of std::mt19937(s) for the seeds first .. first + count - 1 (count a multiple of 256)
hipError_t launch_build_seed_table_range(uint32_t* table, uint32_t first, uint32_t count, hipStream_t stream);
// fills the kSampleWindow rows of the device's sample table (above RenderParams)
hipError_t launch_build_sample_table(float4* table, hipStream_t stream);

// probes
// host_reciprocals: d_count floats in device memory, 1.0f / d as the host rounds it (what the render kernels get)
hipError_t launch_probe_div_const(uint32_t d_first, uint32_t d_count, int mode, const float* host_reciprocals, unsigned long long* counts, hipStream_t stream);
hipError_t launch_probe_intersect(const uint8_t* scene, const float* rays, int n, mcrt_hit* out,
                                  hipStream_t stream);
hipError_t launch_probe_trace(const uint8_t* scene, const mcrt_config& cfg, const float* rays, int n,
                              int depth, float* out, uint32_t* hit_rng, float* deep_stack,
                              hipStream_t stream);
hipError_t launch_probe_mt(const uint32_t* seeds, int n_seeds, int n_draws, float* out, uint32_t* storage,
                           hipStream_t stream);
hipError_t launch_probe_detmath(int op, const float* x, const float* y, size_t n, float* out,
                                hipStream_t stream);
hipError_t launch_probe_detmath_range(int op, uint32_t lo_bits, uint64_t count, float y0, float* out,
                                      hipStream_t stream);

}  // namespace mcrt

#endif
