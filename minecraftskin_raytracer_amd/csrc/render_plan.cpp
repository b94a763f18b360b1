// render_plan.cpp — host-side planning of the launches: shards, the workspace and its batches, grids, plates, batches of
// frames, and the shapes, variants and LDS sizes of the layers, ground, ground-occlusion, reflection, light, bake and skin passes.  Pure host code: what it decides
// reaches the kernels through RenderParams and the other structs of kernels.h; the constants it shares with them are in
// launch_shapes.h.
#include "kernels.h"

#include "flat_scene.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace mcrt {

using rt::kMtShortMax;

Shard make_shard(const mcrt_config& cfg, int first, int step) {
    Shard s{};
    s.first = first;
    s.step = step < 1 ? 1 : step;
    s.pack_first = 0;
    s.pack_step = 1;
    if (cfg.width <= 0 || cfg.height <= 0 || cfg.tile_size <= 0) return s;
    s.tiles_x = (cfg.width + cfg.tile_size - 1) / cfg.tile_size;
    s.tiles_y = (cfg.height + cfg.tile_size - 1) / cfg.tile_size;
    s.owned_rows = (first < s.tiles_y && first >= 0) ? (s.tiles_y - first + s.step - 1) / s.step : 0;
    return s;
}

// development knobs: a positive integer from the environment, read once by the static that holds it
static int int_knob(const char* name, int fallback) {
    const char* e = getenv(name);
    const int v = e ? atoi(e) : 0;
    return v > 0 ? v : fallback;
}

// rare features that need the general kernel variants (one launch set per level, ping-pong queues): per-hit RNG
// streams longer than the register-only engine covers (they run AO inside `level_shade`, sequentially), or
// more bounces than the flat record arrays are laid out for, or extra lights (mcrt.h: the multi-light stages are general ones)
static bool needs_general_variant(const mcrt_config& c, int extra_lights) {
    return extra_lights > 0 || (c.ao_enabled && (c.ao_samples <= 0 || 2 * c.ao_samples > kMtShortMax)) || (soft_sampling(c) && 2 * c.shadow_samples > kMtShortMax) ||
           c.max_bounces > kFlatMaxBounces;
}

// Parts of a tile that meshes can touch: one 256-sample chunk each, at most 16 — fine enough that
// the few tiles holding the character spread over the chip.  Every part reads its samples' draws from
// the tile's stream in HBM (plan_tiles).  Background tiles are never split.
//
// Units by block (p.unit_blocks; not for a renderTile rectangle, which keeps pixel ranges): the tile is cut by a grid of
// gx x gy blocks of ceil(T / gx) x ceil(T / gy) pixels, gx * gy <= 16.  Of the grids whose block is at most one chunk of
// samples and no more than twice as long as it is wide, the one with the FEWEST blocks is taken (the fullest chunks); among
// those the squarest, then the wider one.  8 x 8 blocks at 4 spp on a tile of 16, 24 or 32, 16 x 16 at 1 spp, 16 x 8 at 2 spp
// and 11 x 7 at 3 spp of a tile of 32.  A workgroup's samples then lie in a square patch of the screen instead of a 32 x 2
// strip: their rays meet the same few meshes and the same faces (DESIGN.md §4 "Units by block").  Where no such grid exists
// — more than 4 spp on a tile of 32, where the cap of 16 makes a unit several chunks, or a tile too large — the tile keeps
// its pixel ranges: a chunk of a range is then a few neighbouring pixels already, and blocks only gather the hits into
// fewer units, which the kernels that stride over the units statically (`ao`, `resolve`) pay for (gui_defaults -2.1 %).
static int choose_parts_per_tile(RenderParams& p) {
    const mcrt_config& cfg = p.cfg;
    const long long spp = cfg.samples_per_pixel > 1 ? cfg.samples_per_pixel : 1;
    const long long tile_items = p.rect_w > 0 ? static_cast<long long>(p.rect_w) * p.rect_h * spp : static_cast<long long>(cfg.tile_size) * cfg.tile_size * spp;
    long long parts = (tile_items + kChunk - 1) / kChunk;
    const long long most = p.rect_w > 0 ? 4096 : 16;  // a renderTile rectangle may be as large as the frame: it is the launch's only tile
    if (parts > most) parts = most;
    if (parts < 1) parts = 1;
    p.unit_gx = p.unit_gy = p.unit_bw = p.unit_bh = 0;
    if (p.rect_w > 0 || cfg.tile_size <= 0 || cfg.tile_size > 0xffff) p.unit_blocks = 0;  // (a block's origin and size are 16-bit fields of its record)
    if (!p.unit_blocks) return static_cast<int>(parts);
    const long long T = cfg.tile_size;
    long long best_key = -1;
    for (long long gx = 1; gx <= 16; ++gx)
        for (long long gy = 1; gx * gy <= 16; ++gy) {
            const long long bw = (T + gx - 1) / gx, bh = (T + gy - 1) / gy;
            const long long lo = bw < bh ? bw : bh, hi = bw < bh ? bh : bw;
            if (bw * bh * spp > kChunk || hi > 2 * lo) continue;
            const long long key = ((gx * gy) << 40) | ((hi - lo) << 8) | (bw >= bh ? 0 : 1);  // fewest blocks, then the squarest, then the wider one
            if (best_key < 0 || key < best_key) {
                best_key = key;
                p.unit_gx = static_cast<int>(gx), p.unit_gy = static_cast<int>(gy), p.unit_bw = static_cast<int>(bw), p.unit_bh = static_cast<int>(bh);
            }
        }
    if (best_key < 0) {  // no grid of one chunk per block: pixel ranges
        p.unit_blocks = 0;
        return static_cast<int>(parts);
    }
    return p.unit_gx * p.unit_gy;
}

WorkspaceBytes plan_workspace(RenderParams& p, size_t budget_bytes, const int* row_touched, int extra_lights) {
    WorkspaceBytes w{};
    const mcrt_config& c = p.cfg;
    const int n_tiles = owned_tiles(p);
    p.parts_per_tile = choose_parts_per_tile(p);
    p.flat = needs_general_variant(c, extra_lights) ? 0 : 1;
    const size_t lights = extra_lights > 0 ? static_cast<size_t>(extra_lights) + 1 : 1;  // per record: a disk, a bundle mask and a lit count per light
    p.ws.stack_stride = c.max_bounces > 0 ? c.max_bounces + 1 : 1;
    const size_t spp = c.samples_per_pixel > 1 ? c.samples_per_pixel : 1;
    // every tile that meshes can touch owns one slot per sample of a full (frame-clipped) tile
    const size_t tile_w = p.rect_w > 0 ? static_cast<size_t>(p.rect_w) : static_cast<size_t>(c.tile_size < c.width ? c.tile_size : c.width);
    const size_t tile_h = p.rect_w > 0 ? static_cast<size_t>(p.rect_h) : static_cast<size_t>(c.tile_size < c.height ? c.tile_size : c.height);
    const size_t tile_slots = tile_w * tile_h * spp;
    const size_t S = soft_sampling(c) ? static_cast<size_t>(c.shadow_samples) : 0;
    const size_t A = c.ao_enabled && c.ao_samples > 0 ? static_cast<size_t>(c.ao_samples) : 0;
    const size_t rays = S > A ? S : A;  // light samples and AO directions share one array
    // records per slot: flat — the primary hit and one per reflection level; general — two ping-pong queues
    const size_t recs = p.flat ? static_cast<size_t>(1 + (c.max_bounces > 0 ? c.max_bounces : 0)) : 2;
    // bytes per slot: colour + end code, per record 5 float4 + light samples + mask + lit, AO counts, stack
    // light sample positions and bundle masks in HBM: general variants (per record) and the AO directions of
    // the primary hits; the flat pipeline's `lit` keeps the light samples in LDS
    const size_t hbm_rays = p.flat ? 0 : rays;  // the flat pipeline keeps light samples in LDS and AO directions in registers
    const size_t ray_recs = p.flat ? 1 : recs;
    const size_t per_entry = 16 + 4 + recs * (5 * 16 + 4) + ray_recs * lights * (12 * hbm_rays + (hbm_rays ? 8 : 0) + 4) + 4 + 16 * static_cast<size_t>(p.ws.stack_stride);
    // `lit`: a round is a block of up to 256 records (masks, counts and the list of traced records in LDS); the sample
    // positions of the records whose rays are traced go through an area of kLitLdsBytes, `lit_pass` records at a time
    {
        const size_t pairs = S ? S : 1;
        size_t pass = kLitLdsBytes / (12 * pairs);
        if (pass > static_cast<size_t>(kBlock)) pass = kBlock;
        if (pass < 1) pass = 1;
        p.lit_round = kBlock;
        p.lit_pass = static_cast<int>(pass);
        p.lit_lds_bytes = static_cast<int>(pass * 12 * pairs + static_cast<size_t>(kBlock) * 24);  // positions + (candidates, inside, lit count, traced list) per record of a round
        p.lit_lds_offset = static_cast<int>((scene_table_bytes(p) + 15) & ~static_cast<size_t>(15));
    }
    const int owned = p.shard.owned_rows;
    auto row_count = [&](int j) -> size_t { return row_touched ? static_cast<size_t>(row_touched[j]) : static_cast<size_t>(p.shard.tiles_x); };
    // touched tiles of the fullest batch when the shard is cut into batches of R owned rows
    auto fullest = [&](int R) -> size_t {
        size_t mx = 0;
        for (int r0 = 0; r0 < owned; r0 += R) {
            size_t sum = 0;
            for (int j = r0; j < owned && j < r0 + R; ++j) sum += row_count(j);
            if (sum > mx) mx = sum;
        }
        return mx;
    };
    // the tiles' jitter / lens draws: of the touched tiles only when `plan_tiles` renders the background tiles
    // itself (few draws per pixel: a 624-word twist then completes >= 26 pixels, enough for whole rounds of
    // the wave's 64 lanes), of every tile of the batch otherwise
    const size_t draws_stride = tile_slots * static_cast<size_t>(p.draws_per_sample);
    // A transparent frame takes the touched-tiles layout at every sample count: its background tiles are (0,0,0,0) and need
    // no stream at all, so only the touched tiles' draws exist (no `background_kernel`, no background work in `primary`).
    p.bg_in_plan = (p.background == MCRT_BACKGROUND_TRANSPARENT || spp * static_cast<size_t>(p.draws_per_sample) <= 24) ? 1 : 0;
    static const size_t slab_min_spp = static_cast<size_t>(int_knob("MCRT_SLAB_MIN_SPP", kSlabMinSpp));  // (the parity sweeps run the slab kernel at every sample count with it)
    p.bg_kernel = (!p.bg_in_plan && spp >= slab_min_spp) ? 1 : 0;
    const size_t draws_row_bytes = p.bg_in_plan ? 0 : draws_stride * 4 * static_cast<size_t>(p.shard.tiles_x);
    const size_t draws_tile_bytes = p.bg_in_plan ? draws_stride * 4 : 0;
    p.ws.draws_stride = static_cast<uint32_t>(draws_stride > 0xffffffffull ? 0xffffffffull : draws_stride);
    p.ws.tile_slots = static_cast<uint32_t>(tile_slots > 0xffffffffull ? 0xffffffffull : tile_slots);
    // records are indexed with 32 bits (with room for the 3·S multiplier done in size_t)
    const size_t index_limit = 0x7ffffff0ull / (recs * lights);  // (a record's lights are indexed record * lights + k)
    size_t tile_budget = budget_bytes / (per_entry * (tile_slots ? tile_slots : 1) + draws_tile_bytes);
    if (tile_slots && tile_budget > index_limit / tile_slots) tile_budget = index_limit / tile_slots;
    int rows = owned > 0 ? owned : 1;
    // a batch of R rows fits when its hit workspace and its draws fit the budget together
    auto fits = [&](int R) -> bool {
        const size_t f = fullest(R);
        if (f > tile_budget) return false;
        return f * (tile_slots * per_entry + draws_tile_bytes) + static_cast<size_t>(R) * draws_row_bytes <= budget_bytes;
    };
    if (owned > 0 && !fits(rows)) {  // largest R that fits (monotone in R)
        int lo = 1, hi = owned;
        while (lo < hi) {
            const int mid = (lo + hi + 1) / 2;
            if (fits(mid)) lo = mid; else hi = mid - 1;
        }
        rows = lo;  // a batch is never smaller than one tile row
    }
    size_t cap_tiles = owned > 0 ? fullest(rows) : 0;
    if (cap_tiles < 1) cap_tiles = 1;
    p.rows_per_batch = rows;
    if (tile_slots == 0 || cap_tiles > index_limit / tile_slots || draws_stride > 0xffff0000ull)
        p.rows_per_batch = 0;  // one tile (row) alone exceeds the 32-bit index ranges: refused by the caller
    const size_t cap = p.rows_per_batch ? cap_tiles * tile_slots : 1;
    // (+ 256 x recs: `lit`'s chase regions start at the level-1 count rounded up to a whole block)
    const size_t rec_cap = cap * recs + (p.flat ? static_cast<size_t>(kBlock) * recs : 0);
    p.ws.cap = static_cast<uint32_t>(cap);
    p.ws.tile_cap = static_cast<uint32_t>(cap_tiles);
    {  // the tile streams' parts (tile_stream_wave): four waves per tile unless the stream is too short for that
        static const int parts_knob = int_knob("MCRT_STREAM_PARTS", 0);  // 1 / 2 / 4
        const size_t twists = (draws_stride + 623) / 624;  // of a full tile's stream
        int parts = (parts_knob == 1 || parts_knob == 2 || parts_knob == 4) ? parts_knob : kStreamWaves;
        while (parts > 1 && twists < static_cast<size_t>(2 * parts)) parts >>= 1;  // at least two twists per part
        p.stream_parts = p.draws_per_sample > 0 ? parts : 1;
        p.stream_part_twists = static_cast<int>((twists + static_cast<size_t>(p.stream_parts) - 1) / static_cast<size_t>(p.stream_parts));
        if (p.stream_part_twists < 1) p.stream_part_twists = 1;
    }
    w.tile_rng = p.draws_per_sample > 0 ? static_cast<size_t>(n_tiles) * 624 * 4 * static_cast<size_t>(p.stream_parts) : 0;
    w.tile_draws = static_cast<size_t>(rows) * draws_row_bytes + cap_tiles * draws_tile_bytes;
    w.scol = cap * 16;
    w.end = cap * 4;
    p.ws.unit_cap = static_cast<uint32_t>(cap_tiles * static_cast<size_t>(p.parts_per_tile));
    w.units = static_cast<size_t>(p.ws.unit_cap) * 16;
    w.unit_hits = static_cast<size_t>(p.ws.unit_cap) * 4;
    w.tile_mask = static_cast<size_t>(n_tiles > 0 ? n_tiles : 1) * 8;
    w.queue_each = rec_cap * 16;
    w.texel_refs = p.flat ? rec_cap * 4 : 4;
    w.targets = (p.flat ? cap : rec_cap) * 12 * hbm_rays * lights;
    w.cand = hbm_rays ? (p.flat ? cap : rec_cap) * 8 * lights : 0;
    w.lit0 = p.flat ? 4 : cap * 4 * lights;  // the flat pipeline keeps the lit counts in LDS
    w.lit1 = cap * 4 * lights;
    w.stack = cap * 16 * static_cast<size_t>(p.ws.stack_stride);
    w.counters = (static_cast<size_t>(kCounterWords) * 2 + 4) * 4;  // the counters, their base (the previous pass's last values), frame_info
    w.hit_rng = p.flat ? 0 : static_cast<size_t>(256) * kBlock * 624 * 4;  // general grids are capped at 256 WGs
    return w;
}

// Workgroup caps of a render's launches.  Every kernel strides over device-side counts, so a cap changes nothing but
// the schedule.  A frame alone on the device finishes soonest with many workgroups per kernel (`lit`'s rounds differ in
// cost: 16 per CU balance better than 8, -7 us); frames that share the device — four handles in flight, or the lanes of
// one large frame — get through fastest with FEWER workgroups per kernel (4 per CU), which leaves CU slots to the other
// frames' kernels instead of queueing whole kernels behind each other (+4 % frames/s at 1080p; profiles/r03_experiments/grid_sweep*.txt).
void choose_grids(RenderParams& p, bool shared_device, bool company) {
    static const int queue_knob = int_knob("MCRT_QUEUE_GRID", 0);
    static const int primary_knob = int_knob("MCRT_PRIMARY_GRID", 0),
                     ao_knob = int_knob("MCRT_AO_GRID", queue_knob), lit_knob = int_knob("MCRT_LIT_GRID", queue_knob),
                     resolve_knob = int_knob("MCRT_RESOLVE_GRID", 0);
    p.shared_device = shared_device ? 1 : 0;
    // `plan_tiles`: a tile's stream by as many waves as it has parts when the chain of twists is what the kernel waits for —
    // long streams (64 spp: 210-420 twists per tile; GUI defaults alone 4.50 -> 4.10 ms, 8K 18.2 -> 16.8), or a frame that has
    // no company at all, neither other frames nor lanes of its own (1080p: -7 us) — and by ONE wave otherwise: four times the waves bring four times the tile set-up, state
    // loads and partial rounds and take the slots that other frames' or lanes' kernels would fill (-8 % frames/s at 1080p
    // with four frames in flight, -7 % for 4K / 4 spp on three lanes; profiles/r03_experiments/stream_waves.txt)
    static const int waves_knob = int_knob("MCRT_STREAM_WAVES", 0);  // development knob: 1 / 2 / 4
    const bool long_streams = p.stream_part_twists * p.stream_parts >= 128;
    p.stream_waves = (long_streams || !company) ? p.stream_parts : 1;
    if (waves_knob == 1 || waves_knob == 2 || waves_knob == 4) p.stream_waves = waves_knob < p.stream_parts ? waves_knob : p.stream_parts;
    if (p.stream_waves < 1) p.stream_waves = 1;
    p.grid_primary = primary_knob ? primary_knob : (shared_device ? kSharedGrid : kPrimaryGrid);
    p.grid_ao = ao_knob ? ao_knob : (shared_device ? kSharedGrid : kQueueGrid);
    p.grid_lit = lit_knob ? lit_knob : (shared_device ? kSharedGrid : kLitGridAlone);
    p.grid_resolve = resolve_knob ? resolve_knob : (shared_device ? kSharedGrid : kResolveGrid);
}

// ---- background plate (kernels.h) ---------------------------------------------------------------
bool bg_plate_eligible(const RenderParams& p) {
    return p.background == MCRT_BACKGROUND_REFERENCE && p.cfg.gradient_bg != 0 && p.cfg.samples_per_pixel > 1 && p.bg_in_plan == 1 && p.rect_w <= 0 &&
           p.draws_per_sample > 0;
}
size_t bg_plate_bytes(const mcrt_config& cfg) {
    if (cfg.width <= 0 || cfg.height <= 0 || cfg.tile_size <= 0) return 0;
    const size_t ts = static_cast<size_t>(cfg.tile_size);
    const size_t tiles = ((static_cast<size_t>(cfg.width) + ts - 1) / ts) * ((static_cast<size_t>(cfg.height) + ts - 1) / ts);
    if (ts > 0xffffull || tiles > 0x7fffffffull / (ts * ts)) return 0;
    return tiles * ts * ts * sizeof(float4);
}
RenderParams bg_plate_fill_params(const RenderParams& p) {
    RenderParams q = p;
    q.shard = make_shard(p.cfg, 0, 1);
    q.layout = MCRT_LAYOUT_FRAME;
    q.out = nullptr;
    q.out8 = nullptr;
    q.bg_plate = nullptr;
    q.rect_x = q.rect_y = q.rect_w = q.rect_h = 0;
    return q;
}
size_t bg_plate_rng_bytes(const RenderParams& p) {
    const RenderParams q = bg_plate_fill_params(p);
    return static_cast<size_t>(owned_tiles(q)) * 624 * 4 * static_cast<size_t>(q.stream_parts);
}

// ---- draw plate (kernels.h) -----------------------------------------------------------------------
bool draw_plate_eligible(const RenderParams& p) {
    const int spp = p.cfg.samples_per_pixel > 1 ? p.cfg.samples_per_pixel : 1;
    return p.bg_in_plan == 1 && p.draws_per_sample > 0 && p.rect_w <= 0 && spp * p.draws_per_sample <= 24 && p.ws.draws_stride > 0;
}
size_t draw_plate_bytes(const RenderParams& p) {
    const mcrt_config& cfg = p.cfg;
    if (cfg.width <= 0 || cfg.height <= 0 || cfg.tile_size <= 0 || p.ws.draws_stride == 0) return 0;
    const size_t ts = static_cast<size_t>(cfg.tile_size);
    const size_t tiles = ((static_cast<size_t>(cfg.width) + ts - 1) / ts) * ((static_cast<size_t>(cfg.height) + ts - 1) / ts);
    if (tiles > 0x7fffffffull) return 0;  // (TileGeom::frame_tile is an int)
    return tiles * static_cast<size_t>(p.ws.draws_stride) * sizeof(float);
}
size_t draw_plate_rng_bytes(const RenderParams& p) { return bg_plate_rng_bytes(p); }  // the same whole-frame shard's engine states

// ---- batches ----------------------------------------------------------------------------------
bool batch_eligible(const RenderParams& p) {
    return p.flat && p.rect_w <= 0 && p.shard.owned_rows > 0 && p.rows_per_batch >= p.shard.owned_rows;
}

static int batch_grid(int single, int n_frames) {
    if (n_frames <= 1) return single;
    int g = (kBatchTarget + n_frames - 1) / n_frames;
    if (g < kBatchMinGrid) g = kBatchMinGrid;
    return g < single ? g : single;
}

hipError_t plan_batch(RenderParams* f, int n, bool others_running, BatchPlan& plan) {
    plan = BatchPlan{};
    if (n < 1) return hipErrorInvalidValue;
    const RenderParams& a = f[0];
    bool any_hbm = false, any_posed = false;
    for (int i = 0; i < n; ++i) {
        const RenderParams& q = f[i];
        // the launch shapes are functions of the config: frames that disagree cannot share a launch
        if (!batch_eligible(q) || std::memcmp(&q.cfg, &a.cfg, sizeof(mcrt_config)) != 0 || std::memcmp(&q.shard, &a.shard, sizeof(Shard)) != 0 ||
            q.parts_per_tile != a.parts_per_tile || q.stream_parts != a.stream_parts || q.stream_part_twists != a.stream_part_twists ||
            q.draws_per_sample != a.draws_per_sample || q.bg_in_plan != a.bg_in_plan || q.bg_kernel != a.bg_kernel || q.lit_lds_bytes != a.lit_lds_bytes ||
            q.background != a.background)
            return hipErrorInvalidValue;
        any_hbm = any_hbm || !q.scene_in_lds;
        any_posed = any_posed || q.scene_posed;
    }
    // one variant for the whole batch, the most general any frame needs: kViewHbm > kViewLds > kViewLdsUnposed.  The
    // kernels decide the record layout from p.scene_posed, not from the variant, so a frame under a more general variant
    // renders exactly as alone; under kViewHbm its tables are read from HBM and lit's area starts at offset 0.
    plan.view = any_hbm ? kViewHbm : (any_posed ? kViewLds : kViewLdsUnposed);
    for (int i = 0; i < n; ++i) {
        RenderParams& q = f[i];
        if (any_hbm) {
            q.scene_in_lds = 0, q.lds_alpha_words = 0, q.lds_face_entries = 0;
            q.lit_lds_offset = 0;
        }
        const size_t tables = scene_table_bytes(q);
        if (static_cast<size_t>(q.lit_lds_offset) != ((tables + 15) & ~static_cast<size_t>(15))) return hipErrorInvalidValue;
        plan.dyn = tables > plan.dyn ? tables : plan.dyn;
        const size_t lit = static_cast<size_t>(q.lit_lds_offset) + static_cast<size_t>(q.lit_lds_bytes);
        plan.lit_dyn = lit > plan.lit_dyn ? lit : plan.lit_dyn;
    }
    // grids: what a frame would get with company (the other frames of the batch), then the batch rule above
    const int spp = a.cfg.samples_per_pixel > 1 ? a.cfg.samples_per_pixel : 1;
    const double samples = static_cast<double>(a.shard.owned_rows) * a.cfg.tile_size * a.cfg.width * spp;
    const bool company = n > 1 || others_running;
    for (int i = 0; i < n; ++i) {
        RenderParams& q = f[i];
        choose_grids(q, company && samples < 6.4e7, company);
        q.grid_primary = batch_grid(q.grid_primary, n);
        q.grid_ao = batch_grid(q.grid_ao, n);
        q.grid_lit = batch_grid(q.grid_lit, n);
        q.grid_resolve = batch_grid(q.grid_resolve, n);
    }
    return hipSuccess;
}

// ---- geometry layers (kernels.h) ------------------------------------------------------------------
LdsFit lds_fit(uint32_t alpha_words, uint32_t n_meshes, bool posed) {
    const bool fits = alpha_words <= static_cast<uint32_t>(kAlphaLdsWordsMax) && n_meshes * 6 <= static_cast<uint32_t>(kFaceLdsEntriesMax);
    if (!fits) return LdsFit{0, 0, kViewHbm};
    return LdsFit{static_cast<int>(n_meshes * 6), static_cast<int>(alpha_words), posed ? kViewLds : kViewLdsUnposed};
}
size_t layers_lds_bytes(const LayersFrame& f) { return scene_tables_lds_bytes(f.lds_face_entries, f.lds_alpha_words); }
bool make_layers_shape(const mcrt_config& cfg, LayersShape& shape) {
    std::memset(&shape, 0, sizeof shape);
    shape.cfg = cfg;
    if (cfg.width <= 0 || cfg.height <= 0 || cfg.tile_size <= 0) return true;  // no tiles
    shape.tiles_x = (cfg.width + cfg.tile_size - 1) / cfg.tile_size;
    shape.tiles_y = (cfg.height + cfg.tile_size - 1) / cfg.tile_size;
    const long long tile_px = static_cast<long long>(cfg.tile_size < cfg.width ? cfg.tile_size : cfg.width) * (cfg.tile_size < cfg.height ? cfg.tile_size : cfg.height);
    const long long parts = (tile_px + kBlock - 1) / kBlock;
    if (static_cast<long long>(shape.tiles_x) * shape.tiles_y * parts > 0x7fffffffll) return false;
    shape.parts = static_cast<int>(parts);
    return true;
}
// items of a pass whose `samples` positions or directions (12 bytes each) fit an LDS area of `bytes` at once: 1 .. kBlock
static int pass_items_that_fit(int bytes, int samples) {
    const int fit = bytes / (12 * (samples > 0 ? samples : 1));
    return fit < 1 ? 1 : (fit > kBlock ? kBlock : fit);
}
// ---- ground shadow (kernels.h) --------------------------------------------------------------------
bool make_ground_shape(const mcrt_config& cfg, bool bundle_decisions, bool inside_fast, GroundShape& shape) {
    std::memset(&shape, 0, sizeof shape);
    if (!make_layers_shape(cfg, shape.tiles)) return false;
    shape.samples = soft_sampling(cfg) ? cfg.shadow_samples : 1;
    shape.pass = pass_items_that_fit(kGroundPosBytes, shape.samples);  // 113 samples: 9 pixels per pass
    shape.bundle_decisions = bundle_decisions ? 1 : 0;
    shape.inside_fast = inside_fast ? 1 : 0;
    return true;
}
size_t ground_lds_bytes(const GroundFrame& f, const GroundShape& shape) {
    const size_t tables = scene_tables_lds_span(f.lds_face_entries, f.lds_alpha_words);
    return tables + kGroundFixedBytes + static_cast<size_t>(shape.pass) * shape.samples * 12;
}
// ---- ground occlusion (kernels.h) -------------------------------------------------------------------
bool make_ground_occlusion_shape(const mcrt_config& cfg, bool inside_fast, GroundOcclusionShape& shape) {
    std::memset(&shape, 0, sizeof shape);
    if (!make_layers_shape(cfg, shape.tiles)) return false;
    shape.ao_samples = cfg.ao_samples;
    shape.ao_radius = cfg.ao_radius;
    shape.pass = pass_items_that_fit(kGroundOccDirBytes, cfg.ao_samples);  // 8 samples: 128 pixels per pass; 113 samples: 9
    shape.inside_fast = inside_fast ? 1 : 0;
    return true;
}
// The 12-mesh character (3120 bytes of tables) at 8 samples: 3120 + 8192 + 128 * 96 = 23600 bytes, four workgroups in a CU's
// 160 KiB.  The directions never take more than kGroundOccDirBytes (the pass shrinks with A), so the largest tables the LDS
// views take (28 KiB) make 49152 bytes, below the 64 KiB a workgroup may ask for.
size_t ground_occlusion_lds_bytes(const GroundOcclusionFrame& f, const GroundOcclusionShape& shape) {
    const size_t tables = scene_tables_lds_span(f.lds_face_entries, f.lds_alpha_words);
    return tables + kGroundOccFixedBytes + static_cast<size_t>(shape.pass) * static_cast<size_t>(shape.ao_samples > 0 ? shape.ao_samples : 1) * 12;
}
// ---- ground reflection (kernels.h) ------------------------------------------------------------------
bool make_reflection_shape(const mcrt_config& cfg, bool bundle_decisions, bool inside_fast, bool cull, ReflectionShape& shape) {
    std::memset(&shape, 0, sizeof shape);
    if (!make_layers_shape(cfg, shape.tiles)) return false;
    shape.samples = soft_sampling(cfg) ? cfg.shadow_samples : 1;
    shape.pass = pass_items_that_fit(kReflectPosBytes, shape.samples);  // 8 samples: 85 hits per pass; 113 samples: 6
    shape.max_bounces = cfg.max_bounces;
    shape.bundle_decisions = bundle_decisions ? 1 : 0;
    shape.inside_fast = inside_fast ? 1 : 0;
    shape.cull = cull ? 1 : 0;
    return true;
}
// The 12-mesh character (72 face entries, 204 alpha words: 3120 bytes of tables) at 8 samples: 3120 + 22528 + 85 * 96 = 33808
// bytes, four workgroups in a CU's 160 KiB.  The largest tables the LDS views take (28 KiB) make 59392 bytes, below the 64 KiB
// a workgroup may ask for.
size_t reflection_lds_bytes(const ReflectionFrame& f, const ReflectionShape& shape) {
    const size_t tables = scene_tables_lds_span(f.lds_face_entries, f.lds_alpha_words);
    return tables + kReflectFixedBytes + static_cast<size_t>(shape.pass) * shape.samples * 12;
}
// ---- light layers (kernels.h) -----------------------------------------------------------------------
bool make_shade_shape(const mcrt_config& cfg, bool bundle_decisions, bool inside_fast, ShadeShape& shape) {
    std::memset(&shape, 0, sizeof shape);
    if (!make_layers_shape(cfg, shape.tiles)) return false;
    shape.samples = soft_sampling(cfg) ? cfg.shadow_samples : 1;
    shape.pass = pass_items_that_fit(kShadePosBytes, shape.samples);  // 8 samples: 85 hits per pass; 113 samples: 6
    shape.ao_samples = cfg.ao_samples;
    shape.ao_radius = cfg.ao_radius;
    shape.bundle_decisions = bundle_decisions ? 1 : 0;
    shape.inside_fast = inside_fast ? 1 : 0;
    return true;
}
// The 12-mesh character (72 face entries, 204 alpha words: 3120 bytes of tables) at 8 samples: `shade` 3120 + 18432 + 85 * 96 =
// 29712 bytes, `occlusion` 3120 + 12288 = 15408 bytes: four workgroups of either in a CU's 160 KiB.  The largest tables the LDS
// views take (28 KiB) make 55296 and 40960 bytes, below the 64 KiB a workgroup may ask for.
size_t shade_lds_bytes(const ShadeFrame& f, const ShadeShape& shape) {
    const size_t tables = scene_tables_lds_span(f.lds_face_entries, f.lds_alpha_words);
    return tables + kShadeFixedBytes + static_cast<size_t>(shape.pass) * shape.samples * 12;
}
size_t occlusion_lds_bytes(const ShadeFrame& f) {
    const size_t tables = scene_tables_lds_span(f.lds_face_entries, f.lds_alpha_words);
    return tables + kOcclusionFixedBytes;
}
// ---- light bake (kernels.h) ---------------------------------------------------------------------------
void bake_owner_faces(const uint8_t* blob, std::vector<BakeFace>& out) {
    out.clear();
    const FlatHeader* h = reinterpret_cast<const FlatHeader*>(blob);
    const FlatMesh* fm = reinterpret_cast<const FlatMesh*>(blob + h->mesh_offset);
    for (uint32_t m = 0; m < h->n_meshes; ++m)  // ascending (mesh, face): the stable sort keeps the owner first among equals
        for (int face = 0; face < 6; ++face)
            if (fm[m].tex_off[face] >= 0 && fm[m].tex_w[face] > 0 && fm[m].tex_h[face] > 0)
                out.push_back(BakeFace{fm[m].tex_off[face], fm[m].tex_w[face], fm[m].tex_h[face], static_cast<int32_t>(m * 8 + static_cast<uint32_t>(face))});
    std::stable_sort(out.begin(), out.end(), [](const BakeFace& a, const BakeFace& b) { return a.tex_off < b.tex_off; });
    out.erase(std::unique(out.begin(), out.end(), [](const BakeFace& a, const BakeFace& b) { return a.tex_off == b.tex_off; }), out.end());
}
void make_bake_shape(const mcrt_config& cfg, int grid, bool bundle_decisions, bool inside_fast, int max_texels, BakeShape& shape) {
    std::memset(&shape, 0, sizeof shape);
    shape.grid = grid;
    shape.samples = soft_sampling(cfg) ? cfg.shadow_samples : 1;
    shape.pass = pass_items_that_fit(kBakePosBytes, shape.samples);  // 8 samples: 85 points per pass; 113 samples: 6
    shape.ao_samples = cfg.ao_samples;
    shape.ao_radius = cfg.ao_radius;
    shape.bundle_decisions = bundle_decisions ? 1 : 0;
    shape.inside_fast = inside_fast ? 1 : 0;
    shape.max_units = max_texels > 0 ? (max_texels - 1) / kBlock + 1 : 0;
    shape.geometry = 1, shape.rays = 1;
}
// The 12-mesh character (72 face entries, 204 alpha words: 3120 bytes of tables) at 8 samples: `bake_shade` 3120 + 22528 + 85 * 96 =
// 33808 bytes, `bake_occlusion` 3120 + 16384 = 19504 bytes: four workgroups of either in a CU's 160 KiB.  The largest tables the LDS
// views take (28 KiB) make 59392 and 45056 bytes, below the 64 KiB a workgroup may ask for.
size_t bake_shade_lds_bytes(const BakeFrame& f, const BakeShape& shape) {
    const size_t tables = scene_tables_lds_span(f.lds_face_entries, f.lds_alpha_words);
    return tables + kBakeShadeFixedBytes + static_cast<size_t>(shape.pass) * shape.samples * 12;
}
size_t bake_occlusion_lds_bytes(const BakeFrame& f) {
    const size_t tables = scene_tables_lds_span(f.lds_face_entries, f.lds_alpha_words);
    return tables + kBakeOcclusionFixedBytes;
}
// ---- skins on resident scenes (kernels.h) -----------------------------------------------------------
size_t skin_tables_bytes(int n_texels) { return 256 * sizeof(float) + static_cast<size_t>(n_texels) * sizeof(uint16_t); }
size_t cape_tables_bytes() { return 256 * sizeof(float) + static_cast<size_t>(kCapeTexels) * sizeof(uint16_t); }

}  // namespace mcrt
