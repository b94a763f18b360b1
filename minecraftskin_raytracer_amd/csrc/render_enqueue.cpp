// render_enqueue.cpp — from a scene handle and a config to launches on a stream: workspace planning, lanes, recorded
// launch graphs, the one-frame, batched and layers device paths and their mcrt_*_device entry points.
#include "host_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace mcrt;
using namespace mcrt_host;

namespace {

// The background mode of the renders the calling thread prepares while a BackgroundOverride lives, instead of each handle's
// own (mcrt_scene::background, which is never written here): a studio shot renders its figures transparent whatever the
// handles are set to, and no other thread sees a handle in another mode meanwhile.  -1: none.
thread_local int t_background_override = -1;
struct BackgroundOverride {
    explicit BackgroundOverride(int mode) { t_background_override = mode; }
    ~BackgroundOverride() { t_background_override = -1; }
    BackgroundOverride(const BackgroundOverride&) = delete;
    BackgroundOverride& operator=(const BackgroundOverride&) = delete;
};

int draws_per_sample(const mcrt_config& c) {
    int spp = c.samples_per_pixel > 1 ? c.samples_per_pixel : 1;
    return (spp > 1 ? 2 : 0) + ((c.dof_enabled && c.aperture > 1e-6f) ? 2 : 0);
}

// lanes for a shard: enough work per lane that the extra launches pay (MCRT_LANES forces a count)
int lane_count(const mcrt_scene* s, const mcrt_config& cfg, const Shard& sh) {
    static const int forced = env_int("MCRT_LANES", 0);
    int lanes;
    if (s->forced_lanes > 0) {
        lanes = s->forced_lanes;
    } else if (forced > 0) {
        lanes = forced;
    } else {
        const int spp = cfg.samples_per_pixel > 1 ? cfg.samples_per_pixel : 1;
        const double samples = static_cast<double>(sh.owned_rows) * cfg.tile_size * cfg.width * spp;
        // One lane up to 2.8e7 samples, three above.  With the launch shapes of a frame that is alone on ONE stream (four
        // waves per tile stream, `lit` at 4 096 workgroups: choose_grids) a single lane beats two or three for every frame
        // up to 2560x1440 / 6 spp (1080p / 4 spp alone: 0.189 / 0.224 / 0.215 ms with 1 / 2 / 3 lanes; 1440p / 6 spp: 0.416 /
        // 0.439 / 0.423); 3840x2160 / 4 spp, 3.3e7 samples: 0.515 / 0.511 / 0.496, and the gap widens from there (GUI defaults,
        // 1.3e8: 5.07 / 4.30 / 4.13).  Two lanes never came out first.
        lanes = samples >= 2.8e7 ? 3 : 1;
    }
    lanes = std::min(lanes, kMaxLanes);
    return std::max(1, std::min(lanes, sh.owned_rows));
}

// Upper bound, per owned tile row of `sh`, of the tiles that plan_tiles can find touched by a mesh.
// It repeats the device's test (mesh_touches_tile + the thin-lens dilation) in double precision
// with several pixels of extra margin, so it can only over-count; anything unusual → every tile.
void touched_tiles_per_row(const mcrt_scene* sc, const mcrt_config& cfg, const Shard& sh, std::vector<int>& out) {
    out.assign(static_cast<size_t>(sh.owned_rows > 0 ? sh.owned_rows : 0), sh.tiles_x);
    if (sh.owned_rows <= 0 || sc->host_meshes.size() < sizeof(FlatHeader)) return;
    const FlatHeader* h = reinterpret_cast<const FlatHeader*>(sc->host_meshes.data());
    const FlatMesh* fm = reinterpret_cast<const FlatMesh*>(sc->host_meshes.data() + h->mesh_offset);
    const int n = static_cast<int>(h->n_meshes);
    if (n == 0) {
        std::fill(out.begin(), out.end(), 0);
        return;
    }
    if (!h->cull_ok || n >= 64) return;
    const double W = cfg.width, H = cfg.height, T = cfg.tile_size;
    const double aspect = static_cast<double>(static_cast<float>(cfg.width) / static_cast<float>(cfg.height));
    const bool dof = cfg.dof_enabled && cfg.aperture > 1e-6f;
    const double half_h = h->cam_half_h, half_w = half_h * aspect;
    std::vector<uint8_t> grid(static_cast<size_t>(sh.tiles_x) * sh.tiles_y, 0);
    for (int i = 0; i < n; ++i) {
        const FlatMesh& m = fm[i];
        double u0 = m.screen[0], v0 = m.screen[1], u1 = m.screen[2], v1 = m.screen[3];
        if (!(u0 <= u1) || !std::isfinite(u0 + u1 + v0 + v1)) return;  // no bound: touches every tile
        if (dof) {
            const double focus = cfg.focus_distance > 0.0f ? cfg.focus_distance : h->cam_focus_auto;
            if (!(m.depth[0] > 0.0f) || !(focus > 0.0)) return;
            const double f_lo = 1.0 / focus, f_hi = std::sqrt(1.0 + half_w * half_w + half_h * half_h) / focus;
            const double z_hi = 1.0 / m.depth[0], z_lo = 1.0 / m.depth[1];
            const double d = std::max(std::max(std::fabs(z_hi - f_lo), std::fabs(z_hi - f_hi)),
                                      std::max(std::fabs(z_lo - f_lo), std::fabs(z_lo - f_hi)));
            // the rounding of lens_ray's origin and focus point at the camera's coordinate magnitude (tile_mesh_mask)
            const double err = 4.0 * 1.1920929e-7 * (static_cast<double>(h->mask_slack) / kMaskSlack + focus + cfg.aperture);
            const double rel = err * f_hi * (1.0 + std::sqrt(half_w * half_w + half_h * half_h));
            if (!(rel < 0.045)) return;  // (the device: 0.05)
            const double pad = (cfg.aperture * d / half_h * 1.02 + 1e-3 + (2.0 * rel + err * z_hi) / half_h) * 1.01 + 1e-4;
            if (!(pad < 1e6)) return;
            u0 -= pad, v0 -= pad, u1 += pad, v1 += pad;
        }
        // bound units → pixels: u = (2x/W - 1) * aspect, v = 1 - 2y/H; the device pads tiles by 2 px + 1e-3 (u) / 2e-3 (v)
        const double pad_x = 6.0 + (1e-3 * aspect + 1e-3) * W / (2.0 * aspect) + 1e-3 * W;
        const double pad_y = 6.0 + 2e-3 * H / 2.0 + 1e-3 * H;
        const double xa = (u0 / aspect + 1.0) * W * 0.5 - pad_x, xb = (u1 / aspect + 1.0) * W * 0.5 + pad_x;
        const double ya = (1.0 - v1) * H * 0.5 - pad_y, yb = (1.0 - v0) * H * 0.5 + pad_y;
        if (!std::isfinite(xa + xb + ya + yb)) return;
        if (xb < 0.0 || yb < 0.0 || xa >= W || ya >= H) continue;
        const int tx0 = static_cast<int>(std::max(0.0, std::floor(xa / T))), tx1 = static_cast<int>(std::min<double>(sh.tiles_x - 1, std::floor(xb / T)));
        const int ty0 = static_cast<int>(std::max(0.0, std::floor(ya / T))), ty1 = static_cast<int>(std::min<double>(sh.tiles_y - 1, std::floor(yb / T)));
        for (int ty = ty0; ty <= ty1; ++ty)
            for (int tx = tx0; tx <= tx1; ++tx) grid[static_cast<size_t>(ty) * sh.tiles_x + tx] = 1;
    }
    for (int j = 0; j < sh.owned_rows; ++j) {
        const int ty = sh.first + j * sh.step;
        int c = 0;
        for (int tx = 0; tx < sh.tiles_x; ++tx) c += grid[static_cast<size_t>(ty) * sh.tiles_x + tx];
        out[static_cast<size_t>(j)] = c;
    }
}

// fill RenderParams for lane `li` of `n_lanes` over the shard (first, step) + make sure its
// workspace exists (allocation only when it has to grow)
int prepare(mcrt_scene* sc, int li, int n_lanes, const mcrt_config* cfg, int first, int step, int layout, float* d_out,
            uint8_t* d_out8, RenderParams& p, std::vector<int>* row_touched_out = nullptr, const mcrt_tile* rect = nullptr) {
    Lane* s = &sc->lanes[li];
    std::memset(&p, 0, sizeof p);
    p.scene = static_cast<const uint8_t*>(sc->blob.ptr);
    p.seed_table = sc->seed_table;
    p.seed_table_full = sc->seed_table_full;
    static const bool decisions = !env_off("MCRT_BUNDLE_DECISIONS");  // development knob: =0 traces every hit's shadow rays
    p.bundle_decisions = decisions ? 1 : 0;
    static const bool inside_fast = !env_off("MCRT_INSIDE_FAST");  // development knob: =0 sends every candidate through the general routine
    p.inside_fast = inside_fast ? 1 : 0;
    static const bool work_tickets = !env_off("MCRT_WORK_TICKETS");  // development knob: =0 strides `primary` and `lit` statically over their work lists
    p.work_tickets = work_tickets ? 1 : 0;
    static const bool unit_blocks = !env_off("MCRT_UNIT_BLOCKS");  // development knob: =0 cuts a touched tile into pixel ranges, not blocks
    p.unit_blocks = (unit_blocks && !rect) ? 1 : 0;
    p.cfg = *cfg;
    if (cfg->width > 0 && cfg->height > 0) {
        p.inv_width = 1.0f / static_cast<float>(cfg->width);
        p.inv_height = 1.0f / static_cast<float>(cfg->height);
        static const bool fast_div = !env_off("MCRT_DIV_FRAME");  // development knob: =0 takes the general division everywhere
        p.div_frame = (fast_div && cfg->width <= kDivFrameMax && cfg->height <= kDivFrameMax) ? 1 : 0;
    }
    p.shard = make_shard(*cfg, first + li * step, step * n_lanes);
    p.shard.pack_first = li;
    p.shard.pack_step = n_lanes;
    if (rect) {  // one tile: the rectangle (renderTile); the output holds its pixel rows, packed
        p.rect_x = rect->x, p.rect_y = rect->y, p.rect_w = rect->width, p.rect_h = rect->height;
        p.shard.first = 0, p.shard.step = 1, p.shard.tiles_x = 1, p.shard.tiles_y = 1, p.shard.owned_rows = 1;
        p.shard.pack_first = 0, p.shard.pack_step = 1;
    }
    p.layout = layout;
    p.out = d_out;
    p.out8 = d_out8;
    p.background = rect ? MCRT_BACKGROUND_REFERENCE : (t_background_override >= 0 ? t_background_override : sc->background);  // (plan_workspace picks the draws layout by it)
    p.draws_per_sample = draws_per_sample(*cfg);
    const LdsFit fit = lds_fit(sc->alpha_words, sc->n_meshes, sc->posed);
    p.scene_in_lds = fit.view != kViewHbm ? 1 : 0;
    p.scene_posed = sc->posed ? 1 : 0;
    p.lds_alpha_words = fit.alpha_words;
    p.lds_face_entries = fit.face_entries;
    // The budget bounds the batch size; when the device cannot give that much right now (other
    // allocations, a shared GPU) the budget is halved — down to one tile row per batch — and the
    // lane's buffers are re-planned, instead of failing the render.
    WorkspaceBytes w{};
    std::vector<int> row_touched;
    if (rect)
        row_touched.assign(1, 1);  // the rectangle counts as touched (plan_tiles decides on the device)
    else
        touched_tiles_per_row(sc, *cfg, p.shard, row_touched);
    for (;;) {
        if (!sc->budget) sc->budget = workspace_budget(sc->device);
        w = plan_workspace(p, sc->budget / static_cast<size_t>(n_lanes), row_touched.empty() ? nullptr : row_touched.data(), rect ? 0 : sc->extra.n_extra);
        if (p.rows_per_batch <= 0 && p.shard.owned_rows > 0)
            return fail(MCRT_ERR_INVALID, "one tile row holds more than 2^31 samples (width x tile size x samples per pixel)");
        hipError_t e = hipSuccess;
        auto want = [&](DeviceBuffer& b, size_t bytes) {
            if (e == hipSuccess) e = b.reserve(bytes);
        };
        want(s->tile_rng, w.tile_rng);
        want(s->tile_draws, w.tile_draws);
        want(s->scol, w.scol);
        want(s->end, w.end);
        want(s->units, w.units);
        want(s->tile_mask, w.tile_mask);
        want(s->unit_hits, w.unit_hits);
        for (auto& q : s->queues) want(q, w.queue_each);
        want(s->texel_refs, w.texel_refs);
        want(s->targets, w.targets);
        want(s->cand, w.cand);
        want(s->lit[0], w.lit0);
        want(s->lit[1], w.lit1);
        want(s->stack, w.stack);
        {
            const void* before = s->counters.ptr;
            want(s->counters, w.counters);
            if (e == hipSuccess && s->counters.ptr != before) e = hipMemset(s->counters.ptr, 0, w.counters);  // incl. the sticky overflow word
        }
        want(s->hit_rng, w.hit_rng);
        if (e == hipSuccess) break;
        (void)hipGetLastError();
        if (e != hipErrorOutOfMemory || p.rows_per_batch <= 1 || sc->budget < (static_cast<size_t>(64) << 20))
            return hip_fail(e, "workspace allocation");
        // make room: this lane's partially grown buffers go, then try again with half the budget
        (void)hipDeviceSynchronize();
        for_each_buffer(*s, [](DeviceBuffer& b) { b.release(); });
        sc->budget /= 2;
    }
    if (row_touched_out) *row_touched_out = row_touched;
    p.tile_rng = w.tile_rng ? static_cast<uint32_t*>(s->tile_rng.ptr) : nullptr;
    WaveSpace& ws = p.ws;
    ws.tile_draws = static_cast<float*>(s->tile_draws.ptr);
    ws.scol = static_cast<float4*>(s->scol.ptr);
    ws.end = static_cast<uint32_t*>(s->end.ptr);
    ws.units = static_cast<uint4*>(s->units.ptr);
    ws.tile_mask = static_cast<unsigned long long*>(s->tile_mask.ptr);
    for (int k = 0; k < 2; ++k) {  // [1] = [0] + cap: the second ping-pong queue (general variants) = the deep records (flat pipeline)
        ws.q_o[k] = static_cast<float4*>(s->queues[0].ptr) + static_cast<size_t>(k) * ws.cap;
        ws.q_d[k] = static_cast<float4*>(s->queues[1].ptr) + static_cast<size_t>(k) * ws.cap;
        ws.q_p[k] = static_cast<float4*>(s->queues[2].ptr) + static_cast<size_t>(k) * ws.cap;
        ws.q_n[k] = static_cast<float4*>(s->queues[3].ptr) + static_cast<size_t>(k) * ws.cap;
        ws.q_t[k] = static_cast<float4*>(s->queues[4].ptr) + static_cast<size_t>(k) * ws.cap;
    }
    ws.q_x = static_cast<int32_t*>(s->texel_refs.ptr);
    ws.targets = static_cast<float*>(s->targets.ptr);
    ws.cand = static_cast<unsigned long long*>(s->cand.ptr);
    ws.lit[0] = static_cast<uint32_t*>(s->lit[0].ptr);
    ws.lit[1] = static_cast<uint32_t*>(s->lit[1].ptr);
    ws.unit_hits = static_cast<uint32_t*>(s->unit_hits.ptr);
    ws.stack = static_cast<float4*>(s->stack.ptr);
    ws.counters = static_cast<uint32_t*>(s->counters.ptr);
    ws.counter_base = ws.counters + kCounterWords;
    ws.frame_info = ws.counters + 2 * kCounterWords;
    ws.hit_rng = w.hit_rng ? static_cast<uint32_t*>(s->hit_rng.ptr) : nullptr;
    return MCRT_OK;
}

// the launches of one render on `stream`: lanes fork from and join the stream
// marks: per lane, or nullptr
int launch_lanes(mcrt_scene* s, const RenderParams* p, int n_lanes, hipStream_t stream, const LaunchMarks* marks = nullptr) {
    const LightSet* lights = (s->extra.n_extra > 0 && p[0].rect_w <= 0) ? &s->extra : nullptr;  // (prepare planned the workspace for them)
    if (n_lanes > 1) {
        if (!s->fork) HIP_TRY(hipEventCreateWithFlags(&s->fork, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(s->fork, stream));
        for (int li = 1; li < n_lanes; ++li) {
            Lane& ln = s->lanes[li];
            HIP_TRY(hipStreamWaitEvent(ln.stream, s->fork, 0));
            HIP_TRY(launch_render(p[li], ln.stream, marks ? &marks[li] : nullptr, lights));
            HIP_TRY(hipEventRecord(ln.done, ln.stream));
        }
    }
    HIP_TRY(launch_render(p[0], stream, marks ? &marks[0] : nullptr, lights));
    for (int li = 1; li < n_lanes; ++li) HIP_TRY(hipStreamWaitEvent(stream, s->lanes[li].done, 0));
    return MCRT_OK;
}

// The frame's plates (device_stores.cpp), both kinds in one call, into the n parameter sets of one render.  Where nothing
// twists any more — the touched tiles' draws come from the draw plate, and the background tiles are copied from their plate
// or need no draws (transparent, one colour, one centred sample) — `plan_tiles` reads no engine state: the render then
// carries no tile_rng, and its seeding and advancing launches are never made.
void take_plates(mcrt_scene* s, RenderParams* p, int n, bool capturing, bool count_sighting) {
    acquire_plates(s, p, n, capturing, count_sighting);
    const RenderParams& a = p[0];
    const bool background_twists = a.background == MCRT_BACKGROUND_REFERENCE && a.cfg.gradient_bg != 0 && a.cfg.samples_per_pixel > 1 && !a.bg_plate;
    if (a.draw_plate && !background_twists)
        for (int i = 0; i < n; ++i) p[i].tile_rng = nullptr;
}

RngKey rng_key_of(const RenderParams& p) {
    RngKey k;
    k.ptr = p.tile_rng;
    k.width = p.cfg.width, k.tile_size = p.cfg.tile_size;
    k.first = p.shard.first, k.step = p.shard.step, k.tiles_x = p.shard.tiles_x, k.owned_rows = p.shard.owned_rows;
    k.rect[0] = p.rect_x, k.rect[1] = p.rect_y, k.rect[2] = p.rect_w, k.rect[3] = p.rect_h;
    k.parts = p.stream_parts, k.part_twists = p.stream_part_twists;
    return k;
}

// MCRT_GRAPH=0 turns launch recording off (every render then issues its four launches per lane and pass itself)
bool graphs_enabled() {
    static const bool v = env_int("MCRT_GRAPH", 1) != 0;
    return v;
}

// deepest recursion the workspace is laid out for (one stack slot per level and sample; the general
// variants also keep one queue counter per level)
constexpr int kMaxBounces = 4000;

// The launches of one render, directly or — when the same parameters keep coming — as one replayed
// hipGraph.  The launch sequence of a render is a pure function of its RenderParams (all control flow
// that depends on data lives on the device), so it is recorded once through stream capture on a private
// stream, lanes included, and replayed with a single hipGraphLaunch: ~75 us of launch calls per render
// become one.
int launch_or_replay(mcrt_scene* s, const RenderParams* p, int n_lanes, hipStream_t stream, bool may_record) {
    if (!graphs_enabled() || !may_record) return launch_lanes(s, p, n_lanes, stream);
    ++s->use_clock;
    mcrt_scene::Recorded* slot = nullptr;
    // (a recorded sequence carries the extra lights it was recorded with as kernel arguments: it is replayed only while they hold)
    auto same = [&](const mcrt_scene::Recorded& r) {
        return r.n_lanes == n_lanes && std::memcmp(r.p, p, sizeof(RenderParams) * n_lanes) == 0 && std::memcmp(&r.lights, &s->extra, sizeof(LightSet)) == 0;
    };
    for (auto& r : s->recorded)
        if (r.exec && same(r)) slot = &r;
    if (!slot) {
        // Recording costs tens of milliseconds (capture + instantiation): a parameter set is recorded
        // at its kRecordAt-th sighting, earlier renders launch directly.
        constexpr int kRecordAt = 4;
        mcrt_scene::Recorded* victim = &s->recorded[0];
        for (auto& r : s->recorded) {
            if (!r.exec && same(r)) {
                slot = &r;
                break;
            }
            if (r.last_use < victim->last_use) victim = &r;
        }
        if (!slot) {  // first sighting: remember the parameters
            if (victim->exec) {  // evicting a recorded sequence: an earlier launch of it may still be running
                (void)hipDeviceSynchronize();
                (void)hipGraphExecDestroy(victim->exec);
            }
            if (victim->graph) (void)hipGraphDestroy(victim->graph);
            victim->exec = nullptr;
            victim->graph = nullptr;
            victim->n_lanes = n_lanes;
            victim->sightings = 0;
            std::memcpy(victim->p, p, sizeof(RenderParams) * kMaxLanes);
            victim->lights = s->extra;
            slot = victim;
        }
        slot->last_use = s->use_clock;
        if (++slot->sightings < kRecordAt) return launch_lanes(s, p, n_lanes, stream);
        if (!s->capture_stream) HIP_TRY(hipStreamCreateWithFlags(&s->capture_stream, hipStreamNonBlocking));
        hipError_t e = hipStreamBeginCapture(s->capture_stream, hipStreamCaptureModeThreadLocal);
        if (e == hipSuccess) {
            const int rc = launch_lanes(s, p, n_lanes, s->capture_stream);
            hipGraph_t g = nullptr;
            e = hipStreamEndCapture(s->capture_stream, &g);
            if (rc == MCRT_OK && e == hipSuccess && g) {
                hipGraphExec_t ex = nullptr;
                e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
                if (e == hipSuccess && ex) {
                    slot->graph = g;
                    slot->exec = ex;
                } else {
                    (void)hipGraphDestroy(g);
                }
            } else if (g) {
                (void)hipGraphDestroy(g);
            }
        }
        if (!slot->exec) {  // recording failed: forget it and launch directly
            (void)hipGetLastError();
            slot->n_lanes = 0;
            return launch_lanes(s, p, n_lanes, stream);
        }
    }
    slot->last_use = s->use_clock;
    HIP_TRY(hipGraphLaunch(slot->exec, stream));
    return MCRT_OK;
}

// One handle is one frame in flight: all renders of a handle share its workspace, so they run one after the other whatever
// streams they are given.  Every render that uses the workspace sits between this pair, which owns the handle's `last_done`
// event.  A render being captured into a caller's graph neither waits for nor records handle events (it runs when that
// graph does, not now).  The pass counters run on from render to render (`resolve` leaves their values as the next pass's
// base): no memset per pass.  Only after a render whose launches failed half way are they put back to zero: the counters
// but their last four words (sticky flags, mcrt_scene_check's), and their base with the four words behind it.
constexpr size_t kCounterResetBytes = static_cast<size_t>(kCounterWords - 4) * 4;    // from word 0
constexpr size_t kBaseResetBytes = (static_cast<size_t>(kCounterWords) + 4) * 4;     // from word kCounterWords

// The two halves of the handle's event chain, shared by everything that must run one after the other on a handle — its renders
// (which use its workspace) and its repaints (which write the blob the renders read): `stream` waits for the handle's last such
// work where that was enqueued on another stream, and `last_done` exists afterwards; behind the new work `last_done` is recorded.
int join_handle_chain(mcrt_scene* s, hipStream_t stream) {
    if (s->have_last && s->last_stream != stream) HIP_TRY(hipStreamWaitEvent(stream, s->last_done, 0));
    if (!s->last_done) {
        HIP_TRY(hipEventCreateWithFlags(&s->last_done, hipEventDisableTiming));
        s->busy_probe.store(s->last_done, std::memory_order_release);
    }
    return MCRT_OK;
}
int extend_handle_chain(mcrt_scene* s, hipStream_t stream) {
    HIP_TRY(hipEventRecord(s->last_done, stream));
    s->last_stream = stream;
    s->have_last = true;
    return MCRT_OK;
}

int begin_handle_render(mcrt_scene* s, int n_lanes, hipStream_t stream, bool capturing) {
    if (const int rc = join_handle_chain(s, capturing ? s->last_stream : stream); rc != MCRT_OK) return rc;  // (capturing: no wait, the event alone)
    s->flags_checked = false;
    for (int li = 0; li < n_lanes; ++li) {
        Lane& ln = s->lanes[li];
        if (!ln.counters_dirty || !ln.counters.ptr) continue;
        uint32_t* c = static_cast<uint32_t*>(ln.counters.ptr);
        HIP_TRY(hipMemsetAsync(c, 0, kCounterResetBytes, stream));
        HIP_TRY(hipMemsetAsync(c + kCounterWords, 0, kBaseResetBytes, stream));
        ln.counters_dirty = false;
    }
    return MCRT_OK;
}
// rc: what the render's launches returned.  Failed launches leave the lanes' counters marked; otherwise `last_done` is
// recorded behind them.  Returns rc, or the error of the record.
int end_handle_render(mcrt_scene* s, int n_lanes, hipStream_t stream, int rc, bool capturing) {
    if (rc != MCRT_OK) {
        for (int li = 0; li < n_lanes; ++li) s->lanes[li].counters_dirty = true;
        return rc;
    }
    if (capturing) return MCRT_OK;
    return extend_handle_chain(s, stream);
}

// ---- batches: N frames of one config in one launch sequence (mcrt_render_batch_device) -----------------------------
// one launch sequence for the frames p[0..m) of the handles sc[0..m), all eligible (batch_eligible) and prepared on lane 0
int launch_batch_sequence(mcrt_scene* const* sc, RenderParams* p, int m, int device, hipStream_t stream) {
    BatchPlan plan;
    {
        const bool others = device_shared(sc[0]);
        if (plan_batch(p, m, others, plan) != hipSuccess) return fail(MCRT_ERR_HIP, "internal error: the frames of a batch do not share their launch shapes");
    }
    // the table: the frames' rows, then again the rows of the frames whose tile seeds have to be re-made (they are kept per
    // lane with the key they were made for)
    std::vector<RenderParams> rows;
    rows.reserve(2 * static_cast<size_t>(m));
    rows.assign(p, p + m);
    for (int i = 0; i < m; ++i)
        if (p[i].tile_rng && !(rng_key_of(p[i]) == sc[i]->lanes[0].rng_key)) rows.push_back(p[i]);
    const int n_stale = static_cast<int>(rows.size()) - m;
    for (int i = 0; i < m; ++i)
        if (const int rc = begin_handle_render(sc[i], 1, stream, false); rc != MCRT_OK) return rc;
    TableUpload table;
    if (const int rc = upload_table(device, rows.data(), rows.size() * sizeof(RenderParams), stream, table); rc != MCRT_OK) return rc;
    const RenderParams* d_table = static_cast<const RenderParams*>(table.dev);
    hipError_t e = table.status;
    if (e == hipSuccess && n_stale > 0) e = launch_seed_tiles_batch(rows[static_cast<size_t>(m)], d_table + m, n_stale, stream);
    if (e == hipSuccess) e = launch_render_batch(p[0], plan, d_table, m, stream);
    if (e == hipSuccess) e = table.commit(stream);
    const int rc = e == hipSuccess ? MCRT_OK : hip_fail(e, "batched launches");
    for (int i = 0; i < m; ++i) {
        if (rc == MCRT_OK && p[i].tile_rng) sc[i]->lanes[0].rng_key = rng_key_of(p[i]);  // (unchanged where the seeds were kept)
        const int ended = end_handle_render(sc[i], 1, stream, rc, false);
        if (ended != rc) return ended;
    }
    return rc;
}

// ---- geometry layers: depth / normal / albedo / id planes and pixel picks (mcrt_render_layers_device & co) ----------------
// A layers pass reads the scene blob alone — no workspace, no counters, no events of the handle — so it neither waits for the
// handle's renders nor makes them wait; mcrt_scene_destroy and mcrt_scene_check synchronise the device, which covers it.
// frame `index` of a call: the handle's scene, the planes `index * stride` pixels on; returns the kernel variant it needs
int layers_frame_of(const mcrt_scene* s, const mcrt_layers& out, size_t index, size_t stride, LayersFrame& f) {
    std::memset(&f, 0, sizeof f);
    const size_t off = index * stride;
    f.scene = static_cast<const uint8_t*>(s->blob.ptr);
    f.depth = out.depth ? out.depth + off : nullptr;
    f.normal = out.normal ? reinterpret_cast<float4*>(out.normal) + off : nullptr;
    f.albedo = out.albedo ? reinterpret_cast<float4*>(out.albedo) + off : nullptr;
    f.id = out.id ? reinterpret_cast<int4*>(out.id) + off : nullptr;
    return view_of_frame(f, s->alpha_words, s->n_meshes, s->posed);
}
// the same for a ground pass (mcrt_render_ground_device & co), which also reads the device's seed table through the handle
int ground_frame_of(const mcrt_scene* s, const mcrt_ground& out, float ground_y, size_t index, size_t stride, GroundFrame& f) {
    std::memset(&f, 0, sizeof f);
    const size_t off = index * stride;
    f.scene = static_cast<const uint8_t*>(s->blob.ptr);
    f.visibility = out.visibility ? out.visibility + off : nullptr;
    f.distance = out.distance ? out.distance + off : nullptr;
    f.matte = out.matte ? out.matte + off : nullptr;
    f.seed_table = s->seed_table;
    f.ground_y = ground_y;
    return view_of_frame(f, s->alpha_words, s->n_meshes, s->posed);
}
// and for a ground-occlusion pass (mcrt_render_ground_occlusion_device & co), which reads the table of all seeds where the handle holds it
int ground_occlusion_frame_of(const mcrt_scene* s, const mcrt_ground_occlusion& out, float ground_y, size_t index, size_t stride, GroundOcclusionFrame& f) {
    std::memset(&f, 0, sizeof f);
    const size_t off = index * stride;
    f.scene = static_cast<const uint8_t*>(s->blob.ptr);
    f.occlusion = out.occlusion ? out.occlusion + off : nullptr;
    f.matte = out.matte ? out.matte + off : nullptr;
    f.seed_table_full = s->seed_table_full;
    f.ground_y = ground_y;
    return view_of_frame(f, s->alpha_words, s->n_meshes, s->posed);
}
// and for a reflection pass (mcrt_render_reflection_device & co)
int reflection_frame_of(const mcrt_scene* s, const mcrt_reflection& out, float ground_y, size_t index, size_t stride, ReflectionFrame& f) {
    std::memset(&f, 0, sizeof f);
    const size_t off = index * stride;
    f.scene = static_cast<const uint8_t*>(s->blob.ptr);
    f.rgba = out.rgba ? out.rgba + off * 4 : nullptr;
    f.rgba8 = out.rgba8 ? out.rgba8 + off * 4 : nullptr;
    f.distance = out.distance ? out.distance + off : nullptr;
    f.seed_table = s->seed_table;
    f.ground_y = ground_y;
    return view_of_frame(f, s->alpha_words, s->n_meshes, s->posed);
}
// and for a light pass (mcrt_render_light_device & co), which reads both seed tables
int shade_frame_of(const mcrt_scene* s, const mcrt_light_planes& out, size_t index, size_t stride, ShadeFrame& f) {
    std::memset(&f, 0, sizeof f);
    const size_t off = index * stride;
    f.scene = static_cast<const uint8_t*>(s->blob.ptr);
    f.visibility = out.visibility ? out.visibility + off : nullptr;
    f.occlusion = out.occlusion ? out.occlusion + off : nullptr;
    f.direct = out.direct ? out.direct + off * 4 : nullptr;
    f.seed_table = s->seed_table;
    f.seed_table_full = s->seed_table_full;
    return view_of_frame(f, s->alpha_words, s->n_meshes, s->posed);
}
// and for a light bake (mcrt_bake_light_device & co): the planes `index * stride` TEXELS on, the handle's owner faces behind its blob
int bake_frame_of(const mcrt_scene* s, const mcrt_bake_planes& out, size_t index, size_t stride, BakeFrame& f) {
    std::memset(&f, 0, sizeof f);
    const size_t off = index * stride;
    f.scene = static_cast<const uint8_t*>(s->blob.ptr);
    f.faces = reinterpret_cast<const BakeFace*>(static_cast<const uint8_t*>(s->blob.ptr) + s->bake_faces_offset);
    f.n_faces = s->bake_n_faces;
    f.n_texels = s->n_texels;
    f.position = out.position ? reinterpret_cast<float4*>(out.position + off * 4) : nullptr;
    f.normal = out.normal ? reinterpret_cast<float4*>(out.normal + off * 4) : nullptr;
    f.visibility = out.visibility ? out.visibility + off : nullptr;
    f.occlusion = out.occlusion ? out.occlusion + off : nullptr;
    f.direct = out.direct ? out.direct + off * 4 : nullptr;
    f.seed_table = s->seed_table;
    f.seed_table_full = s->seed_table_full;
    return view_of_frame(f, s->alpha_words, s->n_meshes, s->posed);
}

// and for the two passes under extra lights (mcrt_render_light_multi_device, mcrt_bake_light_multi_device & co): the base record
// (shade_frame_of / bake_frame_of) without its light planes — the occlusion plane travels in a ShadeFrame / BakeFrame of its
// own —, then the handle's lights BY VALUE and the planes per light
template <class Frame, class Planes>
void lights_of_frame(const mcrt_scene* s, const Planes& out, size_t off, Frame& f) {
    f.lights = s->extra;
    for (int k = 0; k < kMaxLights; ++k) {
        f.vis[k] = out.visibility[k] ? out.visibility[k] + off : nullptr;
        f.dir[k] = out.direct[k] ? out.direct[k] + off * 4 : nullptr;
    }
    f.combined = out.combined ? out.combined + off * 4 : nullptr;
}
int shade_lights_frame_of(const mcrt_scene* s, const mcrt_light_planes_multi& out, size_t index, size_t stride, ShadeLightsFrame& f) {
    std::memset(&f, 0, sizeof f);
    const int view = shade_frame_of(s, mcrt_light_planes{nullptr, nullptr, nullptr}, index, stride, f);
    lights_of_frame(s, out, index * stride, f);
    return view;
}
int bake_lights_frame_of(const mcrt_scene* s, const mcrt_bake_planes_multi& out, size_t index, size_t stride, BakeLightsFrame& f) {
    std::memset(&f, 0, sizeof f);
    const int view = bake_frame_of(s, mcrt_bake_planes{out.position, out.normal, nullptr, nullptr, nullptr}, index, stride, f);
    lights_of_frame(s, out, index * stride, f);
    return view;
}

// What the layers and the ground entry points check alike, before any device work (only the last check looks inside the
// handles, at their device index).  run = false with MCRT_OK: zero tiles, nothing is written.
int check_pass_arguments(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, const void* d_out, size_t stride, bool& run, int& device) {
    run = false;
    if (n < 0) return fail(MCRT_ERR_INVALID, "n_frames must be >= 0");
    if (!cfg || !d_out || (n > 0 && !scenes)) return fail(MCRT_ERR_INVALID, "NULL argument");
    for (int i = 0; i < n; ++i)
        if (!scenes[i]) return fail(MCRT_ERR_INVALID, "NULL scene handle in the batch");
    if (n == 0 || !valid_frame(cfg)) return MCRT_OK;
    if (stride < static_cast<size_t>(cfg->width) * static_cast<size_t>(cfg->height))
        return fail(MCRT_ERR_INVALID, "frame_stride_pixels is smaller than width * height");
    device = scenes[0]->device;
    for (int i = 1; i < n; ++i)
        if (scenes[i]->device != device) return fail(MCRT_ERR_INVALID, "the handles of a batch must be on one device");
    run = true;
    return MCRT_OK;
}

// ... and the two light entry points (single- and multi-light planes) ahead of it: `none` is what a call that asks for no plane
// is told; the config checks read the occlusion plane alone
template <class Planes>
int check_light_arguments(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, const Planes* d_out, const char* none, size_t stride, bool& run, int& device) {
    if (cfg && d_out && n >= 0 && no_plane(d_out)) return fail(MCRT_ERR_INVALID, none);
    if (cfg && d_out) {
        const mcrt_light_planes occ = occlusion_alone(d_out);
        if (const int rc = check_light_config(cfg, &occ); rc != MCRT_OK) return rc;
    }
    return check_pass_arguments(scenes, n, cfg, d_out, stride, run, device);
}
// What the two bake entry points check alike (only the last checks look inside the handles: device index and texel count).  No
// frame size enters: what check_pass_arguments checks of the other arguments is checked here.  run = false with MCRT_OK: no
// frame or no texel, nothing is written.
template <class Planes>
int check_bake_arguments(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, int grid, const Planes* d_out, const char* none, size_t stride, bool& run,
                         int& device, int& max_texels) {
    run = false;
    if (n < 0) return fail(MCRT_ERR_INVALID, "n_frames must be >= 0");
    if (!cfg || !d_out || (n > 0 && !scenes)) return fail(MCRT_ERR_INVALID, "NULL argument");
    for (int i = 0; i < n; ++i)
        if (!scenes[i]) return fail(MCRT_ERR_INVALID, "NULL scene handle in the batch");
    if (no_plane(d_out)) return fail(MCRT_ERR_INVALID, none);
    const mcrt_bake_planes occ = occlusion_alone(d_out);
    if (const int rc = check_bake_config(cfg, grid, &occ); rc != MCRT_OK) return rc;
    if (n == 0) return MCRT_OK;
    device = scenes[0]->device;
    max_texels = 0;
    for (int i = 0; i < n; ++i) {
        if (scenes[i]->device != device) return fail(MCRT_ERR_INVALID, "the handles of a batch must be on one device");
        if (scenes[i]->n_texels > 0 && stride < static_cast<size_t>(scenes[i]->n_texels)) return fail(MCRT_ERR_INVALID, "texel_stride is smaller than a scene's texel count");
        max_texels = std::max(max_texels, scenes[i]->n_texels);
    }
    run = max_texels > 0;
    return MCRT_OK;
}

// The launches of such a pass.  One frame: its record travels as a kernel argument (`one`).  More: the records go to a slot
// of the batched renders' table ring (refilled only after the launches that read it) and every kLayersBatchMaxFrames of them
// take one launch (`many`).
template <class Frame, class One, class Many>
int launch_pass(int device, const std::vector<Frame>& frames, hipStream_t stream, const char* what, One one, Many many) {
    const int n = static_cast<int>(frames.size());
    if (n == 1) {
        const hipError_t e = one(frames[0]);
        if (e != hipSuccess) return hip_fail(e, what);
        return MCRT_OK;
    }
    if (stream_capturing(stream))
        return fail(MCRT_ERR_INVALID, "a batch cannot be recorded into a caller's graph (its parameter table is uploaded per call)");
    (void)hipGetLastError();
    TableUpload table;
    if (const int rc = upload_table(device, frames.data(), static_cast<size_t>(n) * sizeof(Frame), stream, table); rc != MCRT_OK) return rc;
    const Frame* d_table = static_cast<const Frame*>(table.dev);
    hipError_t e = table.status;
    for (int c0 = 0; c0 < n && e == hipSuccess; c0 += kLayersBatchMaxFrames) e = many(d_table + c0, std::min(kLayersBatchMaxFrames, n - c0));
    if (e == hipSuccess) e = table.commit(stream);
    if (e != hipSuccess) return hip_fail(e, what);
    return MCRT_OK;
}

// The tail the six pass entry points share, behind their argument checks: the n frame records from frame_of(i, frame) (which
// returns the frame's kernel variant), the batch's variant, the largest dynamic LDS of the pass's one or two kernels over the
// frames (lds_of(frame), PassLds), and the launches: one(frame, view) or many(d_table, m, view, lds).
struct PassLds {
    size_t first = 0, second = 0;
};
template <class Frame, class FrameOf, class LdsOf, class One, class Many>
int enqueue_pass(int device, int n, hipStream_t stream, const char* what, FrameOf frame_of, LdsOf lds_of, One one, Many many) {
    std::vector<Frame> frames(static_cast<size_t>(n));
    std::vector<int> views(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) views[static_cast<size_t>(i)] = frame_of(i, frames[static_cast<size_t>(i)]);
    const int view = batch_view_of(frames.data(), views.data(), n);
    PassLds dyn;
    for (const Frame& f : frames) {
        const PassLds d = lds_of(f);
        dyn.first = std::max(dyn.first, d.first), dyn.second = std::max(dyn.second, d.second);
    }
    return launch_pass(
        device, frames, stream, what, [&](const Frame& f) { return one(f, view); }, [&](const Frame* d_table, int m) { return many(d_table, m, view, dyn); });
}

// the floor passes' heights: one per frame, finite
int check_ground_y(int n, const float* ground_y) {
    if (n > 0 && !ground_y) return fail(MCRT_ERR_INVALID, "NULL argument");
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(ground_y[i])) return fail(MCRT_ERR_INVALID, "ground_y must be finite");
    return MCRT_OK;
}

}  // namespace

namespace mcrt_host {

// workspace budget of a render (bytes, all lanes together); MCRT_WORKSPACE_MB overrides (tests use a
// small value to force multi-batch renders).  By default a third of the scene's device's memory (96 GB of the
// MI355X's 288): the workspace is sized for the worst case of every
// sample hitting (~300 B per sample), buffers only ever grow to what a frame needs, and a frame cut into few large
// batches is much faster than many small ones (4K / 8 bounces / 16 spp: 9.7 ms with 4 GiB, 6.1 ms in one batch).
// (total memory of a device: device_stores.cpp)
size_t workspace_budget(int device) {  // read per scene: tests switch MCRT_WORKSPACE_MB between renders
    const long long mb = env_ll("MCRT_WORKSPACE_MB", 0);
    if (mb > 0) return static_cast<size_t>(mb) << 20;
    // (when the device cannot give that much right now — other allocations, a shared GPU — prepare() halves the budget
    // and re-plans instead of failing)
    return std::max<size_t>(static_cast<size_t>(256) << 20, device_total_memory(device) / 3);
}

int validate_config(const mcrt_config* cfg) {
    if (cfg->max_bounces > kMaxBounces) return fail(MCRT_ERR_INVALID, "max_bounces above 4000 is not supported (one stack slot per level and sample)");
    return MCRT_OK;
}

hipEvent_t next_mark(mcrt_scene* s) {
    if (s->marks_used == s->marks.size()) {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
        s->marks.push_back(e);
    }
    return s->marks[s->marks_used++];
}

int enqueue_render(mcrt_scene* s, const mcrt_config* cfg, int first, int step, int layout, float* d_out, uint8_t* d_out8,
                   hipStream_t stream, bool may_record, std::vector<RowGroup>* groups, const mcrt_tile* rect) {
    Shard whole = make_shard(*cfg, first, step);
    if (rect) whole.owned_rows = 1;
    if (whole.owned_rows <= 0) return MCRT_OK;
    if (validate_config(cfg) != MCRT_OK) return MCRT_ERR_INVALID;
    const int n_lanes = lane_count(s, *cfg, whole);
    if (cfg->ao_enabled && cfg->ao_samples > 0) ensure_full_seed_table(s, stream);
    RenderParams p[kMaxLanes];
    std::memset(p, 0, sizeof p);
    std::vector<int> row_touched[kMaxLanes];
    for (int li = 0; li < n_lanes; ++li) {
        int rc = prepare(s, li, n_lanes, cfg, first, step, layout, d_out, d_out8, p[li], groups ? &row_touched[li] : nullptr, rect);
        if (rc != MCRT_OK) return rc;
        Lane& ln = s->lanes[li];
        if (li > 0 && !ln.stream) {
            HIP_TRY(hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&ln.done, hipEventDisableTiming));
        }
    }
    if (n_lanes > 1 && !s->fork) HIP_TRY(hipEventCreateWithFlags(&s->fork, hipEventDisableTiming));
    const bool capturing = stream_capturing(stream);
    {  // Lanes share the device among themselves; a caller's graph is replayed in circumstances unknown now (no event queries
       // while it records).  Frames of 6.4e7 samples and more keep the large grids: their kernels run for milliseconds,
       // balance counts for more than room for the neighbours (GUI defaults and 4K / 16 spp, 1.3e8 samples: 3.14 / 3.20 ms,
       // 1.49 / 1.48; 8K 17.9 / 18.0; but 4K / 4 spp, 3.3e7 samples: 0.351 / 0.340 ms).
        const int spp = cfg->samples_per_pixel > 1 ? cfg->samples_per_pixel : 1;
        const double samples = static_cast<double>(whole.owned_rows) * cfg->tile_size * cfg->width * spp;
        const bool company = n_lanes > 1 || (!capturing && device_shared(s));
        const bool shared = company && samples < 6.4e7;
        for (int li = 0; li < n_lanes; ++li) choose_grids(p[li], shared, company);
    }
    if (capturing && groups) return fail(MCRT_ERR_INVALID, "row-group events cannot be recorded into a caller's graph");
    // the gradient background tiles are copied from the device's background plate of this frame configuration, the touched tiles'
    // draws read from its draw plate, when it has them (built, if at all, before anything of this render is enqueued; every
    // lane and shard reads the same plates)
    take_plates(s, p, n_lanes, capturing, true);
    if (const int rc = begin_handle_render(s, n_lanes, stream, capturing); rc != MCRT_OK) return rc;
    // the tiles' seeded mt19937 states: kept across renders, re-made (on the caller's stream, ahead of
    // the lanes' fork) only when the frame width, the tile size or the shard changed
    for (int li = 0; li < n_lanes; ++li) {
        if (!p[li].tile_rng) continue;
        Lane& ln = s->lanes[li];
        const RngKey k = rng_key_of(p[li]);
        if (!capturing && k == ln.rng_key) continue;
        HIP_TRY(launch_seed_tiles(p[li], stream));
        ln.rng_key = capturing ? RngKey{} : k;  // a captured seeding pass runs when the caller's graph does, not now
    }
    if (groups) {
        // which rows are final when: a row that holds no touched tile is complete behind plan_tiles (which
        // renders background tiles itself); the rows of a pass behind its resolve; everything at the end
        LaunchMarks marks[kMaxLanes];
        std::vector<hipEvent_t> batch_events[kMaxLanes];
        RowGroup early, late;
        std::vector<RowGroup> per_batch;
        for (int li = 0; li < n_lanes; ++li) {
            const RenderParams& q = p[li];
            const int batches = (q.shard.owned_rows + q.rows_per_batch - 1) / q.rows_per_batch;
            auto row_of = [&](int j) { return q.shard.first + j * q.shard.step; };
            if (batches <= 1) {
                hipEvent_t planned = nullptr;
                if (q.bg_in_plan) {
                    planned = next_mark(s);
                    if (!planned) return fail(MCRT_ERR_HIP, "event creation failed");
                    marks[li].after_plan = planned;
                    early.wait.push_back(planned);
                }
                for (int j = 0; j < q.shard.owned_rows; ++j) {
                    const bool background_only = planned && static_cast<size_t>(j) < row_touched[li].size() && row_touched[li][static_cast<size_t>(j)] == 0;
                    (background_only ? early : late).rows.push_back(row_of(j));
                }
            } else {
                batch_events[li].resize(static_cast<size_t>(batches));
                for (int b = 0; b < batches; ++b) {
                    hipEvent_t e = next_mark(s);
                    if (!e) return fail(MCRT_ERR_HIP, "event creation failed");
                    batch_events[li][static_cast<size_t>(b)] = e;
                    RowGroup g;
                    g.wait.push_back(e);
                    for (int j = b * q.rows_per_batch; j < q.shard.owned_rows && j < (b + 1) * q.rows_per_batch; ++j) g.rows.push_back(row_of(j));
                    per_batch.push_back(std::move(g));
                }
                marks[li].batch_done = batch_events[li].data();
                marks[li].n_batch_done = batches;
            }
        }
        const int rc = end_handle_render(s, n_lanes, stream, launch_lanes(s, p, n_lanes, stream, marks), capturing);
        if (rc == MCRT_OK) {
            late.wait.push_back(s->last_done);
            if (!early.rows.empty()) groups->push_back(std::move(early));
            for (auto& g : per_batch) groups->push_back(std::move(g));
            if (!late.rows.empty()) groups->push_back(std::move(late));
        }
        return rc;
    }
    const int rc = capturing ? launch_lanes(s, p, n_lanes, stream) : launch_or_replay(s, p, n_lanes, stream, may_record);
    return end_handle_render(s, n_lanes, stream, rc, capturing);
}

int render_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, float* d_f32, uint8_t* d_u8, size_t stride, hipStream_t stream) {
    BatchInfo& info = last_batch();
    info = BatchInfo{};
    // argument checks, before any device work (the first ones do not look inside the handles)
    if (n < 0) return fail(MCRT_ERR_INVALID, "n_frames must be >= 0");
    if (!cfg || (n > 0 && !scenes)) return fail(MCRT_ERR_INVALID, "NULL argument");
    for (int i = 0; i < n; ++i)
        if (!scenes[i]) return fail(MCRT_ERR_INVALID, "NULL scene handle in the batch");
    {
        std::vector<mcrt_scene*> sorted(scenes, scenes + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return fail(MCRT_ERR_INVALID, "a scene handle is listed twice (each handle owns one workspace: one frame in flight)");
    }
    if (!d_f32 && !d_u8) return fail(MCRT_ERR_INVALID, "both outputs are NULL");
    if (validate_config(cfg) != MCRT_OK) return MCRT_ERR_INVALID;
    if (n == 0 || !valid_frame(cfg)) return MCRT_OK;  // zero tiles: nothing is written
    if (stride < static_cast<size_t>(cfg->width) * static_cast<size_t>(cfg->height))
        return fail(MCRT_ERR_INVALID, "frame_stride_pixels is smaller than width * height");
    const int device = scenes[0]->device;
    for (int i = 1; i < n; ++i)
        if (scenes[i]->device != device) return fail(MCRT_ERR_INVALID, "the handles of a batch must be on one device");
    HIP_TRY(hipSetDevice(device));
    if (stream_capturing(stream))
        return fail(MCRT_ERR_INVALID, "a batch cannot be recorded into a caller's graph (its parameter table is uploaded per call)");
    (void)hipGetLastError();
    // every frame on lane 0 of its handle, one lane: the batched kernels take it when it fits their envelope.  The frames
    // of a launch sequence share their background mode (it selects the `resolve` kernel): one group per mode.
    std::vector<RenderParams> p(static_cast<size_t>(n));
    std::vector<mcrt_scene*> in_batch[2];
    std::vector<RenderParams> batch_p[2];
    std::vector<int> alone;
    bool plate_sighted = false;
    for (int i = 0; i < n; ++i) {
        mcrt_scene* s = scenes[i];
        if (cfg->ao_enabled && cfg->ao_samples > 0) ensure_full_seed_table(s, stream);  // as the handle's first AO render would
        float* f = d_f32 ? d_f32 + static_cast<size_t>(i) * stride * 4 : nullptr;
        uint8_t* b = d_u8 ? d_u8 + static_cast<size_t>(i) * stride * 4 : nullptr;
        const int rc = prepare(s, 0, 1, cfg, 0, 1, MCRT_LAYOUT_FRAME, f, b, p[static_cast<size_t>(i)]);
        if (rc != MCRT_OK) return rc;
        if (batch_eligible(p[static_cast<size_t>(i)])) {
            // the device's plates of the config, through the handle like a single render's; the batch is ONE sighting of their keys
            take_plates(s, &p[static_cast<size_t>(i)], 1, false, !plate_sighted);
            plate_sighted = true;
            const int mode = p[static_cast<size_t>(i)].background == MCRT_BACKGROUND_TRANSPARENT ? 1 : 0;
            in_batch[mode].push_back(s);
            batch_p[mode].push_back(p[static_cast<size_t>(i)]);
        } else {
            alone.push_back(i);
        }
    }
    for (int mode = 0; mode < 2; ++mode) {
        const int nb = static_cast<int>(in_batch[mode].size());
        for (int c0 = 0; c0 < nb; c0 += kBatchMaxFrames) {  // one launch sequence per kBatchMaxFrames frames
            const int m = std::min(kBatchMaxFrames, nb - c0);
            const int rc = launch_batch_sequence(in_batch[mode].data() + c0, batch_p[mode].data() + c0, m, device, stream);
            if (rc != MCRT_OK) return rc;
            info.frames += m;
            ++info.sequences;
        }
    }
    // the rest (more than one pass, or the general variants) one after the other through the single-frame path
    for (int i : alone) {
        float* f = d_f32 ? d_f32 + static_cast<size_t>(i) * stride * 4 : nullptr;
        uint8_t* b = d_u8 ? d_u8 + static_cast<size_t>(i) * stride * 4 : nullptr;
        const int rc = enqueue_render(scenes[i], cfg, 0, 1, MCRT_LAYOUT_FRAME, f, b, stream);
        if (rc != MCRT_OK) return rc;
        ++info.sequences;
    }
    return MCRT_OK;
}

int render_layers_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, const mcrt_layers* d_out, size_t stride, hipStream_t stream) {
    // argument checks, before any device work
    if (cfg && d_out && n >= 0 && no_plane(d_out)) return fail(MCRT_ERR_INVALID, "all four planes are NULL");
    bool run;
    int device = 0;
    if (const int rc = check_pass_arguments(scenes, n, cfg, d_out, stride, run, device); rc != MCRT_OK || !run) return rc;
    LayersShape shape;
    if (!make_layers_shape(*cfg, shape)) return fail(MCRT_ERR_INVALID, "the frame holds more than 2^31 work units");
    HIP_TRY(hipSetDevice(device));
    return enqueue_pass<LayersFrame>(
        device, n, stream, "layers launches", [&](int i, LayersFrame& f) { return layers_frame_of(scenes[i], *d_out, static_cast<size_t>(i), stride, f); },
        [&](const LayersFrame& f) { return PassLds{layers_lds_bytes(f), 0}; }, [&](const LayersFrame& f, int view) { return launch_layers(f, shape, view, stream); },
        [&](const LayersFrame* d_table, int m, int view, PassLds dyn) { return launch_layers_batch(d_table, m, shape, view, dyn.first, stream); });
}

// ---- ground shadow (mcrt_render_ground_device & co): like a layers pass it reads the scene blob alone — and the device's seed
// table, which lives as long as the handle — so it takes no workspace, no counters and none of the handle's events
int render_ground_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, const float* ground_y, const mcrt_ground* d_out, size_t stride,
                               hipStream_t stream) {
    // argument checks, before any device work
    if (cfg && d_out && n >= 0 && no_plane(d_out)) return fail(MCRT_ERR_INVALID, "all three planes are NULL");
    if (const int rc = check_ground_y(n, ground_y); rc != MCRT_OK) return rc;
    if (cfg && cfg->soft_shadows && cfg->shadow_samples > kGroundMaxSamples)
        return fail(MCRT_ERR_INVALID, "a ground pass takes at most 113 shadow samples (the truncated engine's 227 draws)");
    bool run;
    int device = 0;
    if (const int rc = check_pass_arguments(scenes, n, cfg, d_out, stride, run, device); rc != MCRT_OK || !run) return rc;
    if (const int rc = refuse_extra_lights(scenes, n); rc != MCRT_OK) return rc;
    static const bool decisions = !env_off("MCRT_BUNDLE_DECISIONS");  // the development knobs of `lit` (prepare)
    static const bool inside_fast = !env_off("MCRT_INSIDE_FAST");
    GroundShape shape;
    if (!make_ground_shape(*cfg, decisions, inside_fast, shape)) return fail(MCRT_ERR_INVALID, "the frame holds more than 2^31 work units");
    HIP_TRY(hipSetDevice(device));
    return enqueue_pass<GroundFrame>(
        device, n, stream, "ground launches", [&](int i, GroundFrame& f) { return ground_frame_of(scenes[i], *d_out, ground_y[i], static_cast<size_t>(i), stride, f); },
        [&](const GroundFrame& f) { return PassLds{ground_lds_bytes(f, shape), 0}; }, [&](const GroundFrame& f, int view) { return launch_ground(f, shape, view, stream); },
        [&](const GroundFrame* d_table, int m, int view, PassLds dyn) { return launch_ground_batch(d_table, m, shape, view, dyn.first, stream); });
}

// ---- ground occlusion (mcrt_render_ground_occlusion_device & co): the ground pass's host path with another kernel — the scene
// blob and, where an ambient-occlusion render has built it, the device's table of all seeds (the pass never builds it); no
// workspace, no counters and none of the handle's events
int render_ground_occlusion_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, const float* ground_y, const mcrt_ground_occlusion* d_out,
                                         size_t stride, hipStream_t stream) {
    // argument checks, before any device work
    if (cfg && d_out && n >= 0 && no_plane(d_out)) return fail(MCRT_ERR_INVALID, "both planes are NULL");
    if (const int rc = check_ground_y(n, ground_y); rc != MCRT_OK) return rc;
    if (cfg)
        if (const int rc = check_ground_occlusion_config(cfg); rc != MCRT_OK) return rc;
    bool run;
    int device = 0;
    if (const int rc = check_pass_arguments(scenes, n, cfg, d_out, stride, run, device); rc != MCRT_OK || !run) return rc;
    static const bool inside_fast = !env_off("MCRT_INSIDE_FAST");  // the development knob of `lit` (prepare)
    GroundOcclusionShape shape;
    if (!make_ground_occlusion_shape(*cfg, inside_fast, shape)) return fail(MCRT_ERR_INVALID, "the frame holds more than 2^31 work units");
    HIP_TRY(hipSetDevice(device));
    return enqueue_pass<GroundOcclusionFrame>(
        device, n, stream, "ground occlusion launches",
        [&](int i, GroundOcclusionFrame& f) {
            share_full_seed_table(scenes[i]);
            return ground_occlusion_frame_of(scenes[i], *d_out, ground_y[i], static_cast<size_t>(i), stride, f);
        },
        [&](const GroundOcclusionFrame& f) { return PassLds{ground_occlusion_lds_bytes(f, shape), 0}; },
        [&](const GroundOcclusionFrame& f, int view) { return launch_ground_occlusion(f, shape, view, stream); },
        [&](const GroundOcclusionFrame* d_table, int m, int view, PassLds dyn) { return launch_ground_occlusion_batch(d_table, m, shape, view, dyn.first, stream); });
}

// ---- ground reflection (mcrt_render_reflection_device & co): the ground pass's host path with another kernel — the scene blob
// and the device's seed table, no workspace, no counters and none of the handle's events
int render_reflection_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, const float* ground_y, const mcrt_reflection* d_out,
                                   size_t stride, hipStream_t stream) {
    // argument checks, before any device work
    if (cfg && d_out && n >= 0 && no_plane(d_out)) return fail(MCRT_ERR_INVALID, "all three planes are NULL");
    if (const int rc = check_ground_y(n, ground_y); rc != MCRT_OK) return rc;
    if (cfg && cfg->soft_shadows && cfg->shadow_samples > kGroundMaxSamples)
        return fail(MCRT_ERR_INVALID, "a reflection pass takes at most 113 shadow samples (the truncated engine's 227 draws)");
    if (cfg && cfg->max_bounces > kReflectMaxBounces) return fail(MCRT_ERR_INVALID, "a reflection pass takes at most 8 bounces (its per-lane colour stack)");
    bool run;
    int device = 0;
    if (const int rc = check_pass_arguments(scenes, n, cfg, d_out, stride, run, device); rc != MCRT_OK || !run) return rc;
    if (const int rc = refuse_extra_lights(scenes, n); rc != MCRT_OK) return rc;
    static const bool decisions = !env_off("MCRT_BUNDLE_DECISIONS");  // the development knobs of `lit` (prepare)
    static const bool inside_fast = !env_off("MCRT_INSIDE_FAST");
    static const bool cull = !env_off("MCRT_REFLECT_CULL");  // the pass's own: 0 — every mesh for every tile
    ReflectionShape shape;
    if (!make_reflection_shape(*cfg, decisions, inside_fast, cull, shape)) return fail(MCRT_ERR_INVALID, "the frame holds more than 2^31 work units");
    HIP_TRY(hipSetDevice(device));
    return enqueue_pass<ReflectionFrame>(
        device, n, stream, "reflection launches",
        [&](int i, ReflectionFrame& f) { return reflection_frame_of(scenes[i], *d_out, ground_y[i], static_cast<size_t>(i), stride, f); },
        [&](const ReflectionFrame& f) { return PassLds{reflection_lds_bytes(f, shape), 0}; },
        [&](const ReflectionFrame& f, int view) { return launch_reflection(f, shape, view, stream); },
        [&](const ReflectionFrame* d_table, int m, int view, PassLds dyn) { return launch_reflection_batch(d_table, m, shape, view, dyn.first, stream); });
}

// ---- light layers (mcrt_render_light_device & co): the ground pass's host path with two kernels — `shade` for visibility and
// direct, `occlusion` for that plane — over one frame record.  The occlusion kernel seeds from the device's table of all seeds
// only where an ambient-occlusion render has built it: the pass never builds the 16 GiB table itself.
int render_light_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, const mcrt_light_planes* d_out, size_t stride, hipStream_t stream) {
    // argument checks, before any device work
    bool run;
    int device = 0;
    if (const int rc = check_light_arguments(scenes, n, cfg, d_out, "all three planes are NULL", stride, run, device); rc != MCRT_OK || !run) return rc;
    if (const int rc = refuse_extra_lights(scenes, n); rc != MCRT_OK) return rc;
    static const bool decisions = !env_off("MCRT_BUNDLE_DECISIONS");  // the development knobs of `lit` (prepare)
    static const bool inside_fast = !env_off("MCRT_INSIDE_FAST");
    ShadeShape shape;
    if (!make_shade_shape(*cfg, decisions, inside_fast, shape)) return fail(MCRT_ERR_INVALID, "the frame holds more than 2^31 work units");
    HIP_TRY(hipSetDevice(device));
    const bool shade = d_out->visibility || d_out->direct, occlusion = d_out->occlusion != nullptr;
    return enqueue_pass<ShadeFrame>(
        device, n, stream, "light launches",
        [&](int i, ShadeFrame& f) {
            if (occlusion) share_full_seed_table(scenes[i]);
            return shade_frame_of(scenes[i], *d_out, static_cast<size_t>(i), stride, f);
        },
        [&](const ShadeFrame& f) { return PassLds{shade_lds_bytes(f, shape), occlusion_lds_bytes(f)}; },
        [&](const ShadeFrame& f, int view) { return launch_light(f, shape, view, stream); },
        [&](const ShadeFrame* d_table, int m, int view, PassLds dyn) {
            return launch_light_batch(d_table, m, shape, view, shade, dyn.first, occlusion, dyn.second, stream);
        });
}

// ---- light bake (mcrt_bake_light_device & co): the light pass's host path over the texel pool instead of a frame — two kernels
// over one frame record, the scene blob, the handle's owner faces and the device's seed tables; no workspace, no counters and none
// of the handle's events.
int bake_light_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, int grid, const mcrt_bake_planes* d_out, size_t stride, hipStream_t stream) {
    // argument checks, before any device work
    bool run;
    int device = 0, max_texels = 0;
    if (const int rc = check_bake_arguments(scenes, n, cfg, grid, d_out, "all five planes are NULL", stride, run, device, max_texels); rc != MCRT_OK || !run) return rc;
    if (const int rc = refuse_extra_lights(scenes, n); rc != MCRT_OK) return rc;
    static const bool decisions = !env_off("MCRT_BUNDLE_DECISIONS");  // the development knobs of `lit` (prepare)
    static const bool inside_fast = !env_off("MCRT_INSIDE_FAST");
    BakeShape shape;
    make_bake_shape(*cfg, grid, decisions, inside_fast, max_texels, shape);
    HIP_TRY(hipSetDevice(device));
    const bool shade = d_out->visibility || d_out->direct, occlusion = d_out->occlusion != nullptr;
    return enqueue_pass<BakeFrame>(
        device, n, stream, "bake launches",
        [&](int i, BakeFrame& f) {
            if (occlusion) share_full_seed_table(scenes[i]);
            return bake_frame_of(scenes[i], *d_out, static_cast<size_t>(i), stride, f);
        },
        [&](const BakeFrame& f) { return PassLds{bake_shade_lds_bytes(f, shape), bake_occlusion_lds_bytes(f)}; },
        [&](const BakeFrame& f, int view) { return launch_bake(f, shape, view, stream); },
        [&](const BakeFrame* d_table, int m, int view, PassLds dyn) {
            return launch_bake_batch(d_table, m, shape, view, shade, dyn.first, occlusion, dyn.second, stream);
        });
}

// ---- light layers and bake under extra lights (mcrt_render_light_multi_device, mcrt_bake_light_multi_device & co): the host paths
// of the two passes above with a kernel of their own for the planes that read the lights — `shade_lights` / `bake_shade_lights`
// over records that carry the handle's lights by value — and the single-light passes' occlusion kernel, over a record of its own
// with that plane alone, for the plane that reads none.  The checks are the single-light entries', in their order; nothing
// refuses a handle for its lights.
int render_light_multi_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, const mcrt_light_planes_multi* d_out, size_t stride,
                                    hipStream_t stream) {
    // argument checks, before any device work
    bool run;
    int device = 0;
    if (const int rc = check_light_arguments(scenes, n, cfg, d_out, "all planes are NULL", stride, run, device); rc != MCRT_OK || !run) return rc;
    static const bool decisions = !env_off("MCRT_BUNDLE_DECISIONS");  // the development knobs of `lit` (prepare)
    static const bool inside_fast = !env_off("MCRT_INSIDE_FAST");
    ShadeShape shape;
    if (!make_shade_shape(*cfg, decisions, inside_fast, shape)) return fail(MCRT_ERR_INVALID, "the frame holds more than 2^31 work units");
    HIP_TRY(hipSetDevice(device));
    if (light_plane_asked(d_out)) {
        const int rc = enqueue_pass<ShadeLightsFrame>(
            device, n, stream, "light launches", [&](int i, ShadeLightsFrame& f) { return shade_lights_frame_of(scenes[i], *d_out, static_cast<size_t>(i), stride, f); },
            [&](const ShadeLightsFrame& f) { return PassLds{shade_lds_bytes(f, shape), 0}; },
            [&](const ShadeLightsFrame& f, int view) { return launch_light_multi(f, shape, view, stream); },
            [&](const ShadeLightsFrame* d_table, int m, int view, PassLds dyn) { return launch_light_multi_batch(d_table, m, shape, view, dyn.first, stream); });
        if (rc != MCRT_OK) return rc;
    }
    if (!d_out->occlusion) return MCRT_OK;
    const mcrt_light_planes occ = occlusion_alone(d_out);
    return enqueue_pass<ShadeFrame>(
        device, n, stream, "light launches",
        [&](int i, ShadeFrame& f) {
            share_full_seed_table(scenes[i]);
            return shade_frame_of(scenes[i], occ, static_cast<size_t>(i), stride, f);
        },
        [&](const ShadeFrame& f) { return PassLds{0, occlusion_lds_bytes(f)}; }, [&](const ShadeFrame& f, int view) { return launch_light(f, shape, view, stream); },
        [&](const ShadeFrame* d_table, int m, int view, PassLds dyn) { return launch_light_batch(d_table, m, shape, view, false, 0, true, dyn.second, stream); });
}

int bake_light_multi_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, int grid, const mcrt_bake_planes_multi* d_out, size_t stride,
                                  hipStream_t stream) {
    // argument checks, before any device work
    bool run;
    int device = 0, max_texels = 0;
    if (const int rc = check_bake_arguments(scenes, n, cfg, grid, d_out, "all planes are NULL", stride, run, device, max_texels); rc != MCRT_OK || !run) return rc;
    static const bool decisions = !env_off("MCRT_BUNDLE_DECISIONS");  // the development knobs of `lit` (prepare)
    static const bool inside_fast = !env_off("MCRT_INSIDE_FAST");
    BakeShape shape;
    make_bake_shape(*cfg, grid, decisions, inside_fast, max_texels, shape);
    HIP_TRY(hipSetDevice(device));
    const bool lights = light_plane_asked(d_out);
    if (lights) {  // `bake_shade_lights` writes position and normal too
        const int rc = enqueue_pass<BakeLightsFrame>(
            device, n, stream, "bake launches", [&](int i, BakeLightsFrame& f) { return bake_lights_frame_of(scenes[i], *d_out, static_cast<size_t>(i), stride, f); },
            [&](const BakeLightsFrame& f) { return PassLds{bake_shade_lds_bytes(f, shape), 0}; },
            [&](const BakeLightsFrame& f, int view) { return launch_bake_multi(f, shape, view, stream); },
            [&](const BakeLightsFrame* d_table, int m, int view, PassLds dyn) { return launch_bake_multi_batch(d_table, m, shape, view, dyn.first, stream); });
        if (rc != MCRT_OK || !d_out->occlusion) return rc;
    }
    // what is left is the single-light bake's: the occlusion plane, and position / normal where no plane that reads the lights was asked for
    mcrt_bake_planes rest = occlusion_alone(d_out);
    if (!lights) rest.position = d_out->position, rest.normal = d_out->normal;
    const bool occlusion = rest.occlusion != nullptr;
    return enqueue_pass<BakeFrame>(
        device, n, stream, "bake launches",
        [&](int i, BakeFrame& f) {
            if (occlusion) share_full_seed_table(scenes[i]);
            return bake_frame_of(scenes[i], rest, static_cast<size_t>(i), stride, f);
        },
        [&](const BakeFrame& f) { return PassLds{bake_shade_lds_bytes(f, shape), bake_occlusion_lds_bytes(f)}; },
        [&](const BakeFrame& f, int view) { return launch_bake(f, shape, view, stream); },
        [&](const BakeFrame* d_table, int m, int view, PassLds dyn) { return launch_bake_batch(d_table, m, shape, view, false, dyn.first, occlusion, dyn.second, stream); });
}

// ---- skins on resident scenes (mcrt_scene_set_skin_device & co): one workgroup per handle rewrites the texel pool, the alpha
// predicates and the MESH_OPAQUE bits of its blob.  The blob is what the handle's renders read, so a repaint sits in the
// handle's event chain like a render (join_handle_chain / extend_handle_chain, the halves begin_ / end_handle_render use).
// It uses no workspace and no counters: flags_checked and the lanes stay as they are.
namespace {
const char* const kMixedCapes = "the handles of a batch must all have a cape or all have none";
// what of a repaintable handle's blob (header h) the skin owns: everything but the cape's mesh, its 372 texels and — the skin's
// texel count being a multiple of 16 — its 24 alpha-predicate words
struct SkinCounts {
    int n_texels, n_meshes;
    uint32_t alpha_words;
};
SkinCounts skin_counts(const mcrt_scene* s, const FlatHeader* h) {
    if (!s->has_cape) return SkinCounts{static_cast<int>(h->n_texels), static_cast<int>(h->n_meshes), h->alpha_words};
    return SkinCounts{static_cast<int>(h->n_texels) - kCapeTexels, static_cast<int>(h->n_meshes) - 1, h->alpha_words - static_cast<uint32_t>(kCapeAlphaWords)};
}
}  // namespace

int set_skins_batch_device(mcrt_scene* const* scenes, int n, const uint8_t* d_skins, size_t stride_bytes, hipStream_t stream) {
    // argument checks, before any device work (the first ones do not look inside the handles)
    if (n < 0) return fail(MCRT_ERR_INVALID, "n must be >= 0");
    if (!d_skins || (n > 0 && !scenes)) return fail(MCRT_ERR_INVALID, "NULL argument");
    for (int i = 0; i < n; ++i)
        if (!scenes[i]) return fail(MCRT_ERR_INVALID, "NULL scene handle in the batch");
    if (stride_bytes % 4 != 0) return fail(MCRT_ERR_INVALID, "skin_stride_bytes must be a multiple of 4");
    if ((reinterpret_cast<uintptr_t>(d_skins) & 3u) != 0) return fail(MCRT_ERR_INVALID, "the skin images must be aligned to 4 bytes");
    if (n == 0) return MCRT_OK;
    const int kind = scenes[0]->skin_height, device = scenes[0]->device;
    for (int i = 0; i < n; ++i)
        if (scenes[i]->skin_height != 64 && scenes[i]->skin_height != 32)
            return fail(MCRT_ERR_INVALID, "a handle was not created by mcrt_scene_create_skin (only those hold the full mesh table a repaint writes)");
    for (int i = 1; i < n; ++i)
        if (scenes[i]->skin_height != kind) return fail(MCRT_ERR_INVALID, "the handles of a batch must take images of one size (one skin kind, but for the two 64x64 models)");
    for (int i = 1; i < n; ++i)
        if ((scenes[i]->has_cape != 0) != (scenes[0]->has_cape != 0)) return fail(MCRT_ERR_INVALID, kMixedCapes);
    const size_t image_bytes = static_cast<size_t>(64) * static_cast<size_t>(kind) * 4;
    if (stride_bytes < image_bytes) return fail(MCRT_ERR_INVALID, "skin_stride_bytes is smaller than the skin image");
    for (int i = 1; i < n; ++i)
        if (scenes[i]->device != device) return fail(MCRT_ERR_INVALID, "the handles of a batch must be on one device");
    {
        std::vector<mcrt_scene*> sorted(scenes, scenes + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return fail(MCRT_ERR_INVALID, "a scene handle is listed twice (two images for one blob)");
    }
    HIP_TRY(hipSetDevice(device));
    if (stream_capturing(stream)) return fail(MCRT_ERR_INVALID, "a repaint cannot be recorded into a caller's graph (it takes the handles' events)");
    (void)hipGetLastError();
    // one image size: one blob layout per model.  shapes[k] is the layout of the handles of model k — classic 0, slim 1 — each
    // from the header of the first such handle, the device's tables of its kind with it; a model the batch does not hold takes
    // the other's shape, which no frame then names
    SkinPaintShape shapes[kSkinBatchShapes] = {};
    for (int i = 0; i < n; ++i) {
        const mcrt_scene* s = scenes[i];
        if (s->skin_model < 0 || s->skin_model >= kSkinBatchShapes) return fail(MCRT_ERR_INVALID, "a handle's model is neither classic nor slim");
        SkinPaintShape& shape = shapes[s->skin_model];
        if (shape.tables) continue;
        const FlatHeader* h = reinterpret_cast<const FlatHeader*>(s->host_meshes.data());
        shape.tables = s->skin_tables;
        // (a caped handle: the SKIN's texels, words and meshes — the cape's, behind them, are mcrt_scene_set_cape's, and the
        // kernel's last step would otherwise set the cape mesh's MESH_OPAQUE from a bit no skin texel ever sets)
        const SkinCounts c = skin_counts(s, h);
        shape.n_texels = c.n_texels, shape.n_meshes = c.n_meshes, shape.skin_bytes = static_cast<int>(image_bytes);
        shape.mesh_offset = h->mesh_offset, shape.texel_offset = h->texel_offset, shape.alpha_offset = h->alpha_offset, shape.alpha_words = c.alpha_words;
    }
    for (int k = 0; k < kSkinBatchShapes; ++k)
        if (!shapes[k].tables) shapes[k] = shapes[1 - k];
    std::vector<SkinPaintFrame> frames(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
        mcrt_scene* s = scenes[i];
        SkinPaintFrame& f = frames[static_cast<size_t>(i)];
        f = SkinPaintFrame{};
        f.scene = static_cast<uint8_t*>(s->blob.ptr), f.skin = d_skins + static_cast<size_t>(i) * stride_bytes, f.kind = s->skin_model;
        // every handle of a model has that model's layout: a frame writes n_texels texels and alpha_words words of ITS blob
        const FlatHeader* h = reinterpret_cast<const FlatHeader*>(s->host_meshes.data());
        const SkinPaintShape& shape = shapes[f.kind];
        const SkinCounts c = skin_counts(s, h);
        if (s->skin_tables != shape.tables || c.n_texels != shape.n_texels || c.n_meshes != shape.n_meshes ||
            h->mesh_offset != shape.mesh_offset || h->texel_offset != shape.texel_offset || h->alpha_offset != shape.alpha_offset || c.alpha_words != shape.alpha_words)
            return fail(MCRT_ERR_HIP, "internal error: a handle's blob does not have the layout of its skin kind");
    }
    for (int i = 0; i < n; ++i)
        if (const int rc = join_handle_chain(scenes[i], stream); rc != MCRT_OK) return rc;
    const int rc = launch_pass(
        device, frames, stream, "repaint launches", [&](const SkinPaintFrame& f) { return launch_skin_paint(f, shapes[f.kind], stream); },
        [&](const SkinPaintFrame* d_table, int m) { return launch_skin_paint_batch(d_table, m, shapes, stream); });
    if (rc != MCRT_OK) return rc;
    // Should a record fail half way through the batch (the call then returns the error), the handles before it are chained
    // behind the repaint and the others are not: those keep their earlier `last_done`, which still orders their renders among
    // themselves, and the caller — who got an error — cannot count on the order of this repaint against them.
    for (int i = 0; i < n; ++i)
        if (const int rc = extend_handle_chain(scenes[i], stream); rc != MCRT_OK) return rc;
    return MCRT_OK;
}

// ---- capes on resident scenes (mcrt_scene_set_cape_device & co): one workgroup per caped handle rewrites the cape's texels,
// its alpha predicates and its mesh's MESH_OPAQUE bit.  In the handles' event chains like a skin repaint; no workspace, no
// counters.  d_capes NULL: every cape transparent; stride 0: one image for all.
int set_capes_batch_device(mcrt_scene* const* scenes, int n, const uint8_t* d_capes, size_t stride_bytes, hipStream_t stream) {
    // argument checks, before any device work (they read `device`, `skin_height` and `has_cape` of a handle, nothing else)
    if (n < 0) return fail(MCRT_ERR_INVALID, "n must be >= 0");
    if (n > 0 && !scenes) return fail(MCRT_ERR_INVALID, "NULL argument");
    for (int i = 0; i < n; ++i)
        if (!scenes[i]) return fail(MCRT_ERR_INVALID, "NULL scene handle in the batch");
    if (stride_bytes % 4 != 0) return fail(MCRT_ERR_INVALID, "cape_stride_bytes must be a multiple of 4");
    if ((reinterpret_cast<uintptr_t>(d_capes) & 3u) != 0) return fail(MCRT_ERR_INVALID, "the cape images must be aligned to 4 bytes");
    if (stride_bytes != 0 && stride_bytes < static_cast<size_t>(kCapeImageBytes)) return fail(MCRT_ERR_INVALID, "cape_stride_bytes is smaller than the cape image (64x32 RGBA8), and not 0");
    if (n == 0) return MCRT_OK;
    const int kind = scenes[0]->skin_height, device = scenes[0]->device;
    for (int i = 0; i < n; ++i)
        if (scenes[i]->skin_height != 64 && scenes[i]->skin_height != 32)
            return fail(MCRT_ERR_INVALID, "a handle was not created by mcrt_scene_create_skin_cape (only those hold the cape mesh a cape repaint writes)");
    for (int i = 1; i < n; ++i)
        if ((scenes[i]->has_cape != 0) != (scenes[0]->has_cape != 0)) return fail(MCRT_ERR_INVALID, kMixedCapes);
    if (!scenes[0]->has_cape) return fail(MCRT_ERR_INVALID, "a handle has no cape: create it with mcrt_scene_create_skin_cape");
    for (int i = 1; i < n; ++i)
        if (scenes[i]->skin_height != kind) return fail(MCRT_ERR_INVALID, "the handles of a batch must take images of one size (one skin kind, but for the two 64x64 models)");
    for (int i = 1; i < n; ++i)
        if (scenes[i]->device != device) return fail(MCRT_ERR_INVALID, "the handles of a batch must be on one device");
    {
        std::vector<mcrt_scene*> sorted(scenes, scenes + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return fail(MCRT_ERR_INVALID, "a scene handle is listed twice (two images for one blob)");
    }
    HIP_TRY(hipSetDevice(device));
    if (stream_capturing(stream)) return fail(MCRT_ERR_INVALID, "a repaint cannot be recorded into a caller's graph (it takes the handles' events)");
    (void)hipGetLastError();
    // where the cape lies in each blob, from the handle's own header: behind the skin's texels and words, the last mesh
    CapePaintShape shape{};
    shape.tables = scenes[0]->cape_tables;
    std::vector<CapePaintFrame> frames(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
        const mcrt_scene* s = scenes[i];
        const FlatHeader* h = reinterpret_cast<const FlatHeader*>(s->host_meshes.data());
        CapePaintFrame& f = frames[static_cast<size_t>(i)];
        f = CapePaintFrame{};
        bool ok = s->host_meshes.size() >= sizeof(FlatHeader) && s->cape_tables == shape.tables && shape.tables && h->n_meshes >= 1 &&
                  h->n_texels >= static_cast<uint32_t>(kCapeTexels) && (h->n_texels - kCapeTexels) % 16u == 0 && h->alpha_words == (h->n_texels + 15u) / 16u &&
                  h->texel_offset == h->mesh_offset + h->n_meshes * static_cast<uint32_t>(sizeof(FlatMesh)) && h->alpha_offset == h->texel_offset + h->n_texels * 16u &&
                  h->blob_bytes == h->alpha_offset + h->alpha_words * 4u;
        if (ok) {
            f.scene = static_cast<uint8_t*>(s->blob.ptr);
            f.cape = d_capes ? d_capes + static_cast<size_t>(i) * stride_bytes : nullptr;
            f.flags_offset = h->mesh_offset + (h->n_meshes - 1u) * static_cast<uint32_t>(sizeof(FlatMesh)) + static_cast<uint32_t>(offsetof(FlatMesh, flags));
            f.texel_offset = h->texel_offset + (h->n_texels - static_cast<uint32_t>(kCapeTexels)) * 16u;
            f.alpha_offset = h->alpha_offset + (h->alpha_words - static_cast<uint32_t>(kCapeAlphaWords)) * 4u;
            ok = cape_frame_ok(f);
        }
        if (!ok) return fail(MCRT_ERR_HIP, "internal error: a handle's blob does not have the layout of a caped figure");
    }
    for (int i = 0; i < n; ++i)
        if (const int rc = join_handle_chain(scenes[i], stream); rc != MCRT_OK) return rc;
    const int rc = launch_pass(
        device, frames, stream, "cape repaint launches", [&](const CapePaintFrame& f) { return launch_cape_paint(f, shape, stream); },
        [&](const CapePaintFrame* d_table, int m) { return launch_cape_paint_batch(d_table, m, shape, stream); });
    if (rc != MCRT_OK) return rc;
    for (int i = 0; i < n; ++i)
        if (const int rc = extend_handle_chain(scenes[i], stream); rc != MCRT_OK) return rc;
    return MCRT_OK;
}

// ---- views of resident scenes (mcrt_scene_set_view_device & co): the prefix [FlatHeader][FlatMesh x n] of a repaintable
// handle's blob is flattened on the host for the new pose and look (skin_view_table: the flattener's own code, no texel read),
// the tables of a call travel in ONE asynchronous copy through a slot of the table ring — pinned staging, a device buffer
// that grows on demand, and an event behind the launches that read it, so a later call refills neither too early — and one
// wave per handle writes its table over the blob's prefix, keeping the MESH_OPAQUE bits the skin owns.  The call sits in the
// handles' event chains like a repaint.  Behind the launch the handles' host state follows: host_meshes, posed and the
// remembered view — what touched_tiles_per_row, lds_fit and the passes' views plan from, so a render's RenderParams (and with
// them the recorded launch graph it may replay: launch_or_replay compares every word) are those of a fresh handle at that view.
int set_views_batch_device(mcrt_scene* const* scenes, int n, const float (*poses)[12], const mcrt_scene_desc* const* looks, hipStream_t stream) {
    return set_views_cape_batch_device(scenes, n, poses, looks, nullptr, stream);
}

// The same with a cape angle per caped handle (cape_angles NULL: every handle keeps its own): a caped handle's table is the
// caped figure's (skin_view_table_cape) — one mesh and twelve chunks more, the same kernel.
int set_views_cape_batch_device(mcrt_scene* const* scenes, int n, const float (*poses)[12], const mcrt_scene_desc* const* looks, const float* cape_angles,
                                hipStream_t stream) {
    // argument checks, before any device work (they read `device` and `skin_height` of a handle, nothing else)
    if (n < 0) return fail(MCRT_ERR_INVALID, "n must be >= 0");
    if (n > 0 && !scenes) return fail(MCRT_ERR_INVALID, "NULL argument");
    for (int i = 0; i < n; ++i)
        if (!scenes[i]) return fail(MCRT_ERR_INVALID, "NULL scene handle in the batch");
    if (n == 0) return MCRT_OK;
    const int kind = scenes[0]->skin_height, device = scenes[0]->device;
    for (int i = 0; i < n; ++i)
        if (scenes[i]->skin_height != 64 && scenes[i]->skin_height != 32)
            return fail(MCRT_ERR_INVALID, "a handle was not created by mcrt_scene_create_skin (only those hold the full mesh table a view is flattened for)");
    for (int i = 1; i < n; ++i)
        if (scenes[i]->skin_height != kind) return fail(MCRT_ERR_INVALID, "the handles of a batch must take images of one size (one skin kind, but for the two 64x64 models)");
    for (int i = 1; i < n; ++i)
        if (scenes[i]->device != device) return fail(MCRT_ERR_INVALID, "the handles of a batch must be on one device");
    {
        std::vector<mcrt_scene*> sorted(scenes, scenes + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return fail(MCRT_ERR_INVALID, "a scene handle is listed twice (two views for one blob)");
    }
    const bool caped = scenes[0]->has_cape != 0;
    for (int i = 1; i < n; ++i)
        if ((scenes[i]->has_cape != 0) != caped) return fail(MCRT_ERR_INVALID, kMixedCapes);
    if (cape_angles && !caped) return fail(MCRT_ERR_INVALID, "a cape angle was given for a handle without a cape");
    for (int i = 0; cape_angles && i < n; ++i)
        if (!cape_angle_ok(cape_angles[i])) return fail(MCRT_ERR_INVALID, "cape_angle must be within 0 .. 90 degrees");
    HIP_TRY(hipSetDevice(device));
    if (stream_capturing(stream)) return fail(MCRT_ERR_INVALID, "a view change cannot be recorded into a caller's graph (it takes the handles' events)");
    (void)hipGetLastError();
    // the tables, on the host; each must have the layout of the blob it goes into
    const size_t table_bytes = scenes[0]->host_meshes.size();  // one image size: one prefix layout (the two 64x64 models share it)
    std::vector<uint8_t> staged(static_cast<size_t>(n) * table_bytes), table;
    for (int i = 0; i < n; ++i) {
        const mcrt_scene* s = scenes[i];
        const float* pose = poses ? poses[i] : (s->has_pose ? s->view_pose : nullptr);
        const mcrt_scene_desc* look = (looks && looks[i]) ? looks[i] : (s->has_look ? &s->view_look : nullptr);
        const int made = caped ? skin_view_table_cape(kind, s->skin_model, pose, look, cape_angles ? cape_angles[i] : s->cape_angle, table)
                               : skin_view_table(kind, s->skin_model, pose, look, table);  // the handle's own model
        if (made != MCRT_OK) return made;
        bool same = table_bytes >= sizeof(FlatHeader) && table.size() == table_bytes && s->host_meshes.size() == table_bytes;
        if (same) {
            const FlatHeader* a = reinterpret_cast<const FlatHeader*>(table.data());
            const FlatHeader* b = reinterpret_cast<const FlatHeader*>(s->host_meshes.data());
            same = a->magic == b->magic && a->n_meshes == b->n_meshes && a->n_texels == b->n_texels && a->mesh_offset == b->mesh_offset &&
                   a->texel_offset == b->texel_offset && a->blob_bytes == b->blob_bytes && a->alpha_offset == b->alpha_offset &&
                   a->alpha_words == b->alpha_words && a->texel_offset == table_bytes;
        }
        if (!same) return fail(MCRT_ERR_HIP, "internal error: a view's table does not have the layout of the handle's blob");
        std::memcpy(staged.data() + static_cast<size_t>(i) * table_bytes, table.data(), table_bytes);
    }
    const FlatHeader* h = reinterpret_cast<const FlatHeader*>(scenes[0]->host_meshes.data());
    SceneViewShape shape{};
    shape.mesh_offset = h->mesh_offset, shape.n_meshes = static_cast<int>(h->n_meshes), shape.n_chunks = static_cast<int>(table_bytes / 16);
    if (table_bytes % 16 != 0 || shape.n_chunks > kViewMaxChunks) return fail(MCRT_ERR_HIP, "internal error: a view's table does not fit the kernel's three chunks per lane");
    TableUpload tables;
    if (const int rc = upload_table(device, staged.data(), staged.size(), stream, tables); rc != MCRT_OK) return rc;
    if (tables.status != hipSuccess) return hip_fail(tables.status, "view tables upload");
    std::vector<SceneViewFrame> frames(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
        mcrt_scene* s = scenes[i];
        frames[static_cast<size_t>(i)] = SceneViewFrame{static_cast<uint8_t*>(s->blob.ptr), static_cast<const uint8_t*>(tables.dev) + static_cast<size_t>(i) * table_bytes};
        if (const int rc = join_handle_chain(s, stream); rc != MCRT_OK) return rc;
    }
    int launched = 0;  // handles whose launch was enqueued (a batch beyond kLayersBatchMaxFrames takes several)
    int rc = launch_pass(
        device, frames, stream, "view launches",
        [&](const SceneViewFrame& f) {
            const hipError_t e = launch_scene_view(f, shape, stream);
            if (e == hipSuccess) launched = 1;
            return e;
        },
        [&](const SceneViewFrame* d_table, int m) {
            const hipError_t e = launch_scene_view_batch(d_table, m, shape, stream);
            if (e == hipSuccess) launched += m;
            return e;
        });
    if (launched > 0)
        if (const hipError_t e = tables.commit(stream); e != hipSuccess && rc == MCRT_OK) rc = hip_fail(e, "view launches");
    // the host state of the handles whose blob the device now rewrites, and their chains behind the launch (a handle whose
    // launch was not enqueued keeps its view, its state and its earlier `last_done`)
    for (int i = 0; i < launched; ++i) {
        mcrt_scene* s = scenes[i];
        const uint8_t* t = staged.data() + static_cast<size_t>(i) * table_bytes;
        s->host_meshes.assign(t, t + table_bytes);
        const FlatMesh* fm = reinterpret_cast<const FlatMesh*>(t + shape.mesh_offset);
        s->posed = false;
        for (int m = 0; m < shape.n_meshes; ++m) s->posed = s->posed || (fm[m].flags & MESH_ROTATED) != 0;
        if (poses) {
            s->has_pose = true;
            std::memcpy(s->view_pose, poses[i], sizeof s->view_pose);
        }
        if (looks && looks[i]) {
            s->has_look = true;
            apply_look(&s->view_look, looks[i]);
        }
        if (cape_angles) s->cape_angle = cape_angles[i];
        if (const int chained = extend_handle_chain(s, stream); chained != MCRT_OK && rc == MCRT_OK) rc = chained;
    }
    return rc;
}

// ---- studio shot (mcrt_composite_shot_batch_device & co): the blend is a pass like the ground pass — frame records through
// launch_pass, none of the handles' events — over planes instead of a scene; of a handle it takes the blob's address (the
// header's background colour, read on the device) and the device index
namespace {
// the launches of the blend, behind every check: frame i of the inputs in_stride pixels on, of the outputs out_stride pixels on
int launch_shot_frames(mcrt_scene* const* scenes, int n, int device, const mcrt_config* cfg, const ShotSpec& spec, const mcrt_shot_inputs& in,
                       const float* d_occlusion, size_t in_stride, float* d_f32, uint8_t* d_u8, size_t out_stride, hipStream_t stream) {
    const mcrt_shot* shot = spec.shot;
    const float floor_occlusion = spec.floor_occlusion;
    ShotShape shape;
    std::memset(&shape, 0, sizeof shape);
    shape.cfg = *cfg;
    shape.page = shot->page;
    std::memcpy(shape.page_color, shot->page_color, sizeof shape.page_color);
    shape.shadow_strength = shot->shadow_strength, shape.reflectivity = shot->reflectivity, shape.reflection_fade = shot->reflection_fade;
    shape.floor_occlusion = floor_occlusion;
    std::memcpy(shape.shadow_color, spec.shadow_color, sizeof shape.shadow_color);
    if (!(floor_occlusion > 0.0f)) d_occlusion = nullptr;  // oc = +0 either way: the plane is not read
    std::vector<ShotFrame> frames(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
        ShotFrame& f = frames[static_cast<size_t>(i)];
        std::memset(&f, 0, sizeof f);
        const size_t from = static_cast<size_t>(i) * in_stride, to = static_cast<size_t>(i) * out_stride;
        f.scene = static_cast<const uint8_t*>(scenes[i]->blob.ptr);
        f.figure = in.figure + from * 4;
        f.visibility = in.visibility ? in.visibility + from : nullptr;
        f.reflection = in.reflection ? in.reflection + from * 4 : nullptr;
        f.distance = in.reflection_distance ? in.reflection_distance + from : nullptr;
        f.occlusion = d_occlusion ? d_occlusion + from : nullptr;
        f.out = d_f32 ? d_f32 + to * 4 : nullptr;
        f.out8 = d_u8 ? d_u8 + to * 4 : nullptr;
    }
    // the bounds' identities lie ahead of the blend in the stream, and each launch takes the entries of its frames
    int32_t* d_bounds = spec.bounds ? &spec.bounds[0][0] : nullptr;
    if (d_bounds)
        if (const hipError_t e = launch_shot_bounds_init(d_bounds, n, cfg->width, cfg->height, stream); e != hipSuccess) return hip_fail(e, "shot launches");
    int done = 0;  // frames in the launches so far
    return launch_pass(
        device, frames, stream, "shot launches", [&](const ShotFrame& f) { return launch_shot(f, shape, d_bounds, stream); },
        [&](const ShotFrame* d_table, int m) {
            const hipError_t e = launch_shot_batch(d_table, m, shape, d_bounds ? d_bounds + 4 * static_cast<size_t>(done) : nullptr, stream);
            done += m;
            return e;
        });
}
}  // namespace

int composite_shot_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, const ShotSpec& spec, const mcrt_shot_inputs* d_in,
                                const float* d_occlusion, size_t in_stride, float* d_f32, uint8_t* d_u8, size_t out_stride, hipStream_t stream) {
    const mcrt_shot* shot = spec.shot;
    const float floor_occlusion = spec.floor_occlusion;
    // argument checks, before any device work (only the last one looks inside the handles, at their device index)
    if (n < 0) return fail(MCRT_ERR_INVALID, "n_frames must be >= 0");
    if (!cfg || !shot || !d_in || !d_in->figure || (n > 0 && !scenes)) return fail(MCRT_ERR_INVALID, "NULL argument");
    for (int i = 0; i < n; ++i)
        if (!scenes[i]) return fail(MCRT_ERR_INVALID, "NULL scene handle in the batch");
    if (const int rc = check_shot(spec); rc != MCRT_OK) return rc;
    if (const int rc = check_floor_occlusion(floor_occlusion); rc != MCRT_OK) return rc;
    if (shot->reflection_fade > 0.0f && !d_in->reflection_distance)
        return fail(MCRT_ERR_INVALID, "reflection_distance may be NULL only with reflection_fade == 0");
    if (!d_f32 && !d_u8) return fail(MCRT_ERR_INVALID, "both outputs are NULL");
    if (n == 0 || !valid_frame(cfg)) return MCRT_OK;  // zero tiles: nothing is written
    if (shot_frame_too_large(cfg)) return fail(MCRT_ERR_INVALID, "the frame holds 2^31 pixels or more");
    const size_t px = static_cast<size_t>(cfg->width) * static_cast<size_t>(cfg->height);
    if (in_stride < px) return fail(MCRT_ERR_INVALID, "in_stride_pixels is smaller than width * height");
    if (out_stride < px) return fail(MCRT_ERR_INVALID, "out_stride_pixels is smaller than width * height");
    const int device = scenes[0]->device;
    for (int i = 1; i < n; ++i)
        if (scenes[i]->device != device) return fail(MCRT_ERR_INVALID, "the handles of a batch must be on one device");
    if (const int rc = refuse_extra_lights(scenes, n); rc != MCRT_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    if (stream_capturing(stream)) return fail(MCRT_ERR_INVALID, "a shot cannot be recorded into a caller's graph");
    (void)hipGetLastError();
    return launch_shot_frames(scenes, n, device, cfg, spec, *d_in, d_occlusion, in_stride, d_f32, d_u8, out_stride, stream);
}

// Render + ground + reflection + ground occlusion + blend, all on `stream` in order.  The render goes through render_batch_device (the handles'
// event chains, batched kernels where the frames fit them) under the transparent override; the passes and the blend follow it
// in stream order and take no events.  Nothing is forked beside the render.
int render_shot_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, const ShotSpec& spec, const float* ground_y, void* d_scratch,
                             size_t scratch_bytes, float* d_f32, uint8_t* d_u8, size_t stride, hipStream_t stream) {
    const mcrt_shot* shot = spec.shot;
    const float floor_occlusion = spec.floor_occlusion;
    // argument checks, before any device work (only the last ones look inside the handles, at their device index)
    if (n < 0) return fail(MCRT_ERR_INVALID, "n_frames must be >= 0");
    if (!cfg || !shot || (n > 0 && (!scenes || !ground_y))) return fail(MCRT_ERR_INVALID, "NULL argument");
    for (int i = 0; i < n; ++i)
        if (!scenes[i]) return fail(MCRT_ERR_INVALID, "NULL scene handle in the batch");
    if (const int rc = check_shot(spec); rc != MCRT_OK) return rc;
    if (const int rc = check_floor_occlusion(floor_occlusion); rc != MCRT_OK) return rc;
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(ground_y[i])) return fail(MCRT_ERR_INVALID, "ground_y must be finite");
    if (!d_f32 && !d_u8) return fail(MCRT_ERR_INVALID, "both outputs are NULL");
    {
        std::vector<mcrt_scene*> sorted(scenes, scenes + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return fail(MCRT_ERR_INVALID, "a scene handle is listed twice (each handle owns one workspace: one frame in flight)");
    }
    if (const int rc = check_shot_config(cfg, shot, floor_occlusion); rc != MCRT_OK) return rc;
    if (n == 0 || !valid_frame(cfg)) return MCRT_OK;  // zero tiles: nothing is written
    if (shot_frame_too_large(cfg)) return fail(MCRT_ERR_INVALID, "the frame holds 2^31 pixels or more");
    const size_t px = static_cast<size_t>(cfg->width) * static_cast<size_t>(cfg->height);
    if (stride < px) return fail(MCRT_ERR_INVALID, "frame_stride_pixels is smaller than width * height");
    const ShotScratch at = shot_scratch(cfg, shot, n, floor_occlusion);
    if (!d_scratch) return fail(MCRT_ERR_INVALID, "d_scratch is NULL");
    if ((reinterpret_cast<uintptr_t>(d_scratch) & 15u) != 0) return fail(MCRT_ERR_INVALID, "d_scratch is not 16-byte aligned");
    if (scratch_bytes < at.bytes)
        return fail(MCRT_ERR_INVALID, spec.ex                  ? "scratch_bytes is smaller than mcrt_shot_scratch_bytes_ex"
                                      : floor_occlusion > 0.0f ? "scratch_bytes is smaller than mcrt_shot_scratch_bytes_occ"
                                                               : "scratch_bytes is smaller than mcrt_shot_scratch_bytes");
    const int device = scenes[0]->device;
    for (int i = 1; i < n; ++i)
        if (scenes[i]->device != device) return fail(MCRT_ERR_INVALID, "the handles of a batch must be on one device");
    if (const int rc = refuse_extra_lights(scenes, n); rc != MCRT_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    if (stream_capturing(stream)) return fail(MCRT_ERR_INVALID, "a shot cannot be recorded into a caller's graph");
    (void)hipGetLastError();
    char* base = static_cast<char*>(d_scratch);
    auto plane = [&](size_t offset) { return offset == SIZE_MAX ? nullptr : reinterpret_cast<float*>(base + offset); };
    mcrt_shot_inputs in{};
    in.figure = plane(at.figure);
    in.visibility = plane(at.visibility);
    in.reflection = plane(at.reflection);
    in.reflection_distance = plane(at.distance);
    {
        const BackgroundOverride transparent(MCRT_BACKGROUND_TRANSPARENT);
        if (const int rc = render_batch_device(scenes, n, cfg, plane(at.figure), nullptr, px, stream); rc != MCRT_OK) return rc;
    }
    if (in.visibility) {
        mcrt_ground g{};
        g.visibility = plane(at.visibility);
        if (const int rc = render_ground_batch_device(scenes, n, cfg, ground_y, &g, px, stream); rc != MCRT_OK) return rc;
    }
    if (in.reflection) {
        mcrt_reflection r{};
        r.rgba = plane(at.reflection);
        r.distance = plane(at.distance);
        if (const int rc = render_reflection_batch_device(scenes, n, cfg, ground_y, &r, px, stream); rc != MCRT_OK) return rc;
    }
    if (at.occlusion != SIZE_MAX) {
        mcrt_ground_occlusion o{};
        o.occlusion = plane(at.occlusion);
        if (const int rc = render_ground_occlusion_batch_device(scenes, n, cfg, ground_y, &o, px, stream); rc != MCRT_OK) return rc;
    }
    return launch_shot_frames(scenes, n, device, cfg, spec, in, plane(at.occlusion), px, d_f32, d_u8, stride, stream);
}

}  // namespace mcrt_host

extern "C" {

int mcrt_scene_set_skin_device(mcrt_scene* s, const uint8_t* d_skin_rgba8, void* stream) {
    if (!s || !d_skin_rgba8) return fail(MCRT_ERR_INVALID, "NULL argument");
    mcrt_scene* one[1] = {s};
    const size_t image_bytes = static_cast<size_t>(64) * static_cast<size_t>(s->skin_height > 0 ? s->skin_height : 0) * 4;  // (the kind is checked there)
    return set_skins_batch_device(one, 1, d_skin_rgba8, image_bytes, static_cast<hipStream_t>(stream));
}

int mcrt_scene_set_skins_batch_device(mcrt_scene* const* scenes, int n, const uint8_t* d_skins, size_t skin_stride_bytes, void* stream) {
    return set_skins_batch_device(scenes, n, d_skins, skin_stride_bytes, static_cast<hipStream_t>(stream));
}

int mcrt_scene_set_skin(mcrt_scene* s, const uint8_t* skin_rgba8) {
    if (!s || !skin_rgba8) return fail(MCRT_ERR_INVALID, "NULL argument");
    if (s->skin_height != 64 && s->skin_height != 32)
        return fail(MCRT_ERR_INVALID, "the handle was not created by mcrt_scene_create_skin (only those hold the full mesh table a repaint writes)");
    const size_t bytes = static_cast<size_t>(64) * static_cast<size_t>(s->skin_height) * 4;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(s->skin.reserve(bytes));
    // (a second upload into s->skin may not overtake the repaint that reads the first: this call waits for its own)
    HIP_TRY(hipMemcpy(s->skin.ptr, skin_rgba8, bytes, hipMemcpyHostToDevice));
    const int rc = mcrt_scene_set_skin_device(s, static_cast<const uint8_t*>(s->skin.ptr), nullptr);
    if (rc != MCRT_OK) return rc;
    HIP_TRY(hipEventSynchronize(s->last_done));
    return MCRT_OK;
}

int mcrt_scene_set_cape_device(mcrt_scene* s, const uint8_t* d_cape_rgba8, void* stream) {
    if (!s) return fail(MCRT_ERR_INVALID, "NULL argument");
    mcrt_scene* one[1] = {s};
    return set_capes_batch_device(one, 1, d_cape_rgba8, static_cast<size_t>(kCapeImageBytes), static_cast<hipStream_t>(stream));
}

int mcrt_scene_set_capes_batch_device(mcrt_scene* const* scenes, int n, const uint8_t* d_capes, size_t cape_stride_bytes, void* stream) {
    return set_capes_batch_device(scenes, n, d_capes, cape_stride_bytes, static_cast<hipStream_t>(stream));
}

int mcrt_scene_set_cape(mcrt_scene* s, const uint8_t* cape_rgba8) {
    if (!s) return fail(MCRT_ERR_INVALID, "NULL argument");
    if ((s->skin_height != 64 && s->skin_height != 32) || !s->has_cape)
        return fail(MCRT_ERR_INVALID, "the handle has no cape: create it with mcrt_scene_create_skin_cape");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(s->cape.reserve(static_cast<size_t>(kCapeImageBytes)));
    // (a second upload into s->cape may not overtake the repaint that reads the first: this call waits for its own)
    if (cape_rgba8)
        HIP_TRY(hipMemcpy(s->cape.ptr, cape_rgba8, static_cast<size_t>(kCapeImageBytes), hipMemcpyHostToDevice));
    else
        HIP_TRY(hipMemset(s->cape.ptr, 0, static_cast<size_t>(kCapeImageBytes)));  // no cape: zeros
    const int rc = mcrt_scene_set_cape_device(s, static_cast<const uint8_t*>(s->cape.ptr), nullptr);
    if (rc != MCRT_OK) return rc;
    HIP_TRY(hipEventSynchronize(s->last_done));
    return MCRT_OK;
}

int mcrt_scene_set_view_cape_device(mcrt_scene* s, const float pose[12], const mcrt_scene_desc* look, const float* cape_angle, void* stream) {
    if (!s) return fail(MCRT_ERR_INVALID, "NULL argument");
    mcrt_scene* one[1] = {s};
    const mcrt_scene_desc* one_look[1] = {look};
    return set_views_cape_batch_device(one, 1, reinterpret_cast<const float(*)[12]>(pose), one_look, cape_angle, static_cast<hipStream_t>(stream));
}

int mcrt_scene_set_views_cape_batch_device(mcrt_scene* const* scenes, int n, const float (*poses)[12], const mcrt_scene_desc* const* looks, const float* cape_angles,
                                           void* stream) {
    return set_views_cape_batch_device(scenes, n, poses, looks, cape_angles, static_cast<hipStream_t>(stream));
}

int mcrt_scene_set_view_cape(mcrt_scene* s, const float pose[12], const mcrt_scene_desc* look, const float* cape_angle) {
    const int rc = mcrt_scene_set_view_cape_device(s, pose, look, cape_angle, nullptr);
    if (rc != MCRT_OK) return rc;
    HIP_TRY(hipEventSynchronize(s->last_done));
    return MCRT_OK;
}

int mcrt_scene_set_view_device(mcrt_scene* s, const float pose[12], const mcrt_scene_desc* look, void* stream) {
    if (!s) return fail(MCRT_ERR_INVALID, "NULL argument");
    mcrt_scene* one[1] = {s};
    const mcrt_scene_desc* one_look[1] = {look};
    return set_views_batch_device(one, 1, reinterpret_cast<const float(*)[12]>(pose), one_look, static_cast<hipStream_t>(stream));
}

int mcrt_scene_set_views_batch_device(mcrt_scene* const* scenes, int n, const float (*poses)[12], const mcrt_scene_desc* const* looks, void* stream) {
    return set_views_batch_device(scenes, n, poses, looks, static_cast<hipStream_t>(stream));
}

int mcrt_scene_set_view(mcrt_scene* s, const float pose[12], const mcrt_scene_desc* look) {
    const int rc = mcrt_scene_set_view_device(s, pose, look, nullptr);
    if (rc != MCRT_OK) return rc;
    HIP_TRY(hipEventSynchronize(s->last_done));
    return MCRT_OK;
}

int mcrt_render_device(mcrt_scene* s, const mcrt_config* cfg, int first, int step, int layout, float* d_out,
                       void* stream) {
    return mcrt_render_device_ex(s, cfg, first, step, layout, d_out, nullptr, stream);
}

int mcrt_render_device_ex(mcrt_scene* s, const mcrt_config* cfg, int first, int step, int layout, float* d_out_f32,
                          uint8_t* d_out_rgba8, void* stream) {
    if (!s || !cfg || (!d_out_f32 && !d_out_rgba8)) return fail(MCRT_ERR_INVALID, "NULL argument");
    if (!valid_frame(cfg)) return MCRT_OK;  // zero tiles
    if (first < 0 || step < 1) return fail(MCRT_ERR_INVALID, "tile_row_first must be >= 0 and tile_row_step >= 1");
    HIP_TRY(hipSetDevice(s->device));
    return enqueue_render(s, cfg, first, step, layout, d_out_f32, d_out_rgba8, static_cast<hipStream_t>(stream));
}

int mcrt_time_render_device(mcrt_scene* s, const mcrt_config* cfg, int first, int step, int layout, float* d_out,
                            void* stream, int iters, float* avg_render_ms) {
    if (!s || !cfg || !d_out || iters < 1) return fail(MCRT_ERR_INVALID, "bad argument");
    if (!valid_frame(cfg)) return fail(MCRT_ERR_INVALID, "empty frame");
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    double sum = 0.0;
    for (int i = 0; i < iters; ++i) {
        // the events bracket the whole pipeline of the frame (fork, every lane, join) on `stream`
        HIP_TRY(hipEventRecord(s->ev[0], st));
        int rc = enqueue_render(s, cfg, first, step, layout, d_out, nullptr, st);
        if (rc != MCRT_OK) return rc;
        HIP_TRY(hipEventRecord(s->ev[3], st));
        HIP_TRY(hipEventSynchronize(s->ev[3]));
        float a = 0;
        HIP_TRY(hipEventElapsedTime(&a, s->ev[0], s->ev[3]));
        sum += a;
    }
    if (avg_render_ms) *avg_render_ms = static_cast<float>(sum / iters);
    return MCRT_OK;
}

int mcrt_unpack_rows_device(const mcrt_config* cfg, int first, int step, const float* d_packed, float* d_frame,
                            void* stream) {
    if (!cfg || !d_packed || !d_frame) return fail(MCRT_ERR_INVALID, "NULL argument");
    if (!valid_frame(cfg)) return MCRT_OK;
    Shard sh = make_shard(*cfg, first, step);
    HIP_TRY(launch_unpack_rows(*cfg, sh, d_packed, d_frame, static_cast<hipStream_t>(stream)));
    return MCRT_OK;
}

int mcrt_assemble_frame_device(const mcrt_config* cfg, int world, const float* d_gathered, size_t rank_stride_pixels,
                               float* d_frame, void* stream) {
    if (!cfg || !d_gathered || !d_frame || world < 1) return fail(MCRT_ERR_INVALID, "bad argument");
    if (!valid_frame(cfg)) return MCRT_OK;
    const int tiles_y = (cfg->height + cfg->tile_size - 1) / cfg->tile_size;
    const size_t need = static_cast<size_t>((tiles_y + world - 1) / world) * cfg->tile_size * cfg->width;
    if (world > 1 && rank_stride_pixels < need) return fail(MCRT_ERR_INVALID, "rank stride smaller than a rank's packed rows");
    HIP_TRY(launch_assemble_frame(*cfg, world, d_gathered, rank_stride_pixels, d_frame, static_cast<hipStream_t>(stream)));
    return MCRT_OK;
}

int mcrt_quantize_rgba8_device(const float* d_rgba, uint8_t* d_out, size_t n_pixels, void* stream) {
    if (!d_rgba || !d_out) return fail(MCRT_ERR_INVALID, "NULL argument");
    HIP_TRY(launch_quantize(d_rgba, d_out, n_pixels, static_cast<hipStream_t>(stream)));
    return MCRT_OK;
}

int mcrt_render_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, float* d_out_f32, uint8_t* d_out_rgba8,
                             size_t frame_stride_pixels, void* stream) {
    return render_batch_device(scenes, n_frames, cfg, d_out_f32, d_out_rgba8, frame_stride_pixels, static_cast<hipStream_t>(stream));
}

int mcrt_render_layers_device(mcrt_scene* s, const mcrt_config* cfg, const mcrt_layers* d_out, void* stream) {
    if (!s) return fail(MCRT_ERR_INVALID, "NULL argument");
    mcrt_scene* one[1] = {s};
    const size_t px = (cfg && valid_frame(cfg)) ? static_cast<size_t>(cfg->width) * static_cast<size_t>(cfg->height) : 0;
    return render_layers_batch_device(one, 1, cfg, d_out, px, static_cast<hipStream_t>(stream));
}

int mcrt_render_layers_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_layers* d_out,
                                    size_t frame_stride_pixels, void* stream) {
    return render_layers_batch_device(scenes, n_frames, cfg, d_out, frame_stride_pixels, static_cast<hipStream_t>(stream));
}

int mcrt_render_ground_device(mcrt_scene* s, const mcrt_config* cfg, float ground_y, const mcrt_ground* d_out, void* stream) {
    if (!s) return fail(MCRT_ERR_INVALID, "NULL argument");
    mcrt_scene* one[1] = {s};
    const size_t px = (cfg && valid_frame(cfg)) ? static_cast<size_t>(cfg->width) * static_cast<size_t>(cfg->height) : 0;
    return render_ground_batch_device(one, 1, cfg, &ground_y, d_out, px, static_cast<hipStream_t>(stream));
}

int mcrt_render_ground_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const float* ground_y, const mcrt_ground* d_out,
                                    size_t frame_stride_pixels, void* stream) {
    return render_ground_batch_device(scenes, n_frames, cfg, ground_y, d_out, frame_stride_pixels, static_cast<hipStream_t>(stream));
}

int mcrt_render_ground_occlusion_device(mcrt_scene* s, const mcrt_config* cfg, float ground_y, const mcrt_ground_occlusion* d_out, void* stream) {
    if (!s) return fail(MCRT_ERR_INVALID, "NULL argument");
    mcrt_scene* one[1] = {s};
    const size_t px = (cfg && valid_frame(cfg)) ? static_cast<size_t>(cfg->width) * static_cast<size_t>(cfg->height) : 0;
    return render_ground_occlusion_batch_device(one, 1, cfg, &ground_y, d_out, px, static_cast<hipStream_t>(stream));
}

int mcrt_render_ground_occlusion_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const float* ground_y,
                                              const mcrt_ground_occlusion* d_out, size_t frame_stride_pixels, void* stream) {
    return render_ground_occlusion_batch_device(scenes, n_frames, cfg, ground_y, d_out, frame_stride_pixels, static_cast<hipStream_t>(stream));
}

int mcrt_render_reflection_device(mcrt_scene* s, const mcrt_config* cfg, float ground_y, const mcrt_reflection* d_out, void* stream) {
    if (!s) return fail(MCRT_ERR_INVALID, "NULL argument");
    mcrt_scene* one[1] = {s};
    const size_t px = (cfg && valid_frame(cfg)) ? static_cast<size_t>(cfg->width) * static_cast<size_t>(cfg->height) : 0;
    return render_reflection_batch_device(one, 1, cfg, &ground_y, d_out, px, static_cast<hipStream_t>(stream));
}

int mcrt_render_reflection_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const float* ground_y,
                                        const mcrt_reflection* d_out, size_t frame_stride_pixels, void* stream) {
    return render_reflection_batch_device(scenes, n_frames, cfg, ground_y, d_out, frame_stride_pixels, static_cast<hipStream_t>(stream));
}

int mcrt_composite_shot_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_shot* shot, const mcrt_shot_inputs* d_in,
                                     size_t in_stride_pixels, float* d_out_f32, uint8_t* d_out_rgba8, size_t out_stride_pixels, void* stream) {
    return composite_shot_batch_device(scenes, n_frames, cfg, shot_spec(shot, 0.0f), d_in, nullptr, in_stride_pixels, d_out_f32, d_out_rgba8, out_stride_pixels,
                                       static_cast<hipStream_t>(stream));
}

int mcrt_composite_shot_batch_device_occ(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_shot* shot, const mcrt_shot_inputs* d_in,
                                         const float* d_occlusion, float floor_occlusion, size_t in_stride_pixels, float* d_out_f32, uint8_t* d_out_rgba8,
                                         size_t out_stride_pixels, void* stream) {
    return composite_shot_batch_device(scenes, n_frames, cfg, shot_spec(shot, floor_occlusion), d_in, d_occlusion, in_stride_pixels, d_out_f32, d_out_rgba8,
                                       out_stride_pixels, static_cast<hipStream_t>(stream));
}

int mcrt_render_shot_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_shot* shot, const float* ground_y, void* d_scratch,
                                  size_t scratch_bytes, float* d_out_f32, uint8_t* d_out_rgba8, size_t frame_stride_pixels, void* stream) {
    return render_shot_batch_device(scenes, n_frames, cfg, shot_spec(shot, 0.0f), ground_y, d_scratch, scratch_bytes, d_out_f32, d_out_rgba8, frame_stride_pixels,
                                    static_cast<hipStream_t>(stream));
}

int mcrt_render_shot_batch_device_occ(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_shot* shot, float floor_occlusion,
                                      const float* ground_y, void* d_scratch, size_t scratch_bytes, float* d_out_f32, uint8_t* d_out_rgba8,
                                      size_t frame_stride_pixels, void* stream) {
    return render_shot_batch_device(scenes, n_frames, cfg, shot_spec(shot, floor_occlusion), ground_y, d_scratch, scratch_bytes, d_out_f32, d_out_rgba8,
                                    frame_stride_pixels, static_cast<hipStream_t>(stream));
}

int mcrt_render_shot_device(mcrt_scene* s, const mcrt_config* cfg, const mcrt_shot* shot, float ground_y, void* d_scratch, size_t scratch_bytes,
                            float* d_out_f32, uint8_t* d_out_rgba8, void* stream) {
    if (!s || !cfg) return fail(MCRT_ERR_INVALID, "NULL argument");
    mcrt_scene* one[1] = {s};
    const size_t px = valid_frame(cfg) ? static_cast<size_t>(cfg->width) * static_cast<size_t>(cfg->height) : 0;
    return render_shot_batch_device(one, 1, cfg, shot_spec(shot, 0.0f), &ground_y, d_scratch, scratch_bytes, d_out_f32, d_out_rgba8, px, static_cast<hipStream_t>(stream));
}

// the _ex entries: the same paths with the shot's additions in the spec (a NULL shot is refused there, as the others' is)
int mcrt_composite_shot_batch_device_ex(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_shot_ex* shot, const mcrt_shot_inputs* d_in,
                                        const float* d_occlusion, size_t in_stride_pixels, float* d_out_f32, uint8_t* d_out_rgba8, size_t out_stride_pixels,
                                        int32_t (*d_bounds)[4], void* stream) {
    return composite_shot_batch_device(scenes, n_frames, cfg, shot_spec_ex(shot, d_bounds), d_in, d_occlusion, in_stride_pixels, d_out_f32, d_out_rgba8,
                                       out_stride_pixels, static_cast<hipStream_t>(stream));
}

int mcrt_render_shot_batch_device_ex(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_shot_ex* shot, const float* ground_y,
                                     void* d_scratch, size_t scratch_bytes, float* d_out_f32, uint8_t* d_out_rgba8, size_t frame_stride_pixels,
                                     int32_t (*d_bounds)[4], void* stream) {
    return render_shot_batch_device(scenes, n_frames, cfg, shot_spec_ex(shot, d_bounds), ground_y, d_scratch, scratch_bytes, d_out_f32, d_out_rgba8,
                                    frame_stride_pixels, static_cast<hipStream_t>(stream));
}

int mcrt_render_light_device(mcrt_scene* s, const mcrt_config* cfg, const mcrt_light_planes* d_out, void* stream) {
    if (!s) return fail(MCRT_ERR_INVALID, "NULL argument");
    mcrt_scene* one[1] = {s};
    const size_t px = cfg ? static_cast<size_t>(cfg->width > 0 ? cfg->width : 0) * static_cast<size_t>(cfg->height > 0 ? cfg->height : 0) : 0;
    return render_light_batch_device(one, 1, cfg, d_out, px, static_cast<hipStream_t>(stream));
}

int mcrt_render_light_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_light_planes* d_out,
                                   size_t frame_stride_pixels, void* stream) {
    return render_light_batch_device(scenes, n_frames, cfg, d_out, frame_stride_pixels, static_cast<hipStream_t>(stream));
}

int mcrt_bake_light_device(mcrt_scene* s, const mcrt_config* cfg, int grid, const mcrt_bake_planes* d_out, void* stream) {
    if (!s) return fail(MCRT_ERR_INVALID, "NULL argument");
    mcrt_scene* one[1] = {s};
    return bake_light_batch_device(one, 1, cfg, grid, d_out, ~static_cast<size_t>(0), static_cast<hipStream_t>(stream));  // (one frame: no stride)
}

int mcrt_bake_light_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, int grid, const mcrt_bake_planes* d_out,
                                 size_t texel_stride, void* stream) {
    return bake_light_batch_device(scenes, n_frames, cfg, grid, d_out, texel_stride, static_cast<hipStream_t>(stream));
}

int mcrt_render_light_multi_device(mcrt_scene* s, const mcrt_config* cfg, const mcrt_light_planes_multi* d_out, void* stream) {
    if (!s) return fail(MCRT_ERR_INVALID, "NULL argument");
    mcrt_scene* one[1] = {s};
    const size_t px = cfg ? static_cast<size_t>(cfg->width > 0 ? cfg->width : 0) * static_cast<size_t>(cfg->height > 0 ? cfg->height : 0) : 0;
    return render_light_multi_batch_device(one, 1, cfg, d_out, px, static_cast<hipStream_t>(stream));
}

int mcrt_render_light_multi_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, const mcrt_light_planes_multi* d_out,
                                         size_t frame_stride_pixels, void* stream) {
    return render_light_multi_batch_device(scenes, n_frames, cfg, d_out, frame_stride_pixels, static_cast<hipStream_t>(stream));
}

int mcrt_bake_light_multi_device(mcrt_scene* s, const mcrt_config* cfg, int grid, const mcrt_bake_planes_multi* d_out, void* stream) {
    if (!s) return fail(MCRT_ERR_INVALID, "NULL argument");
    mcrt_scene* one[1] = {s};
    return bake_light_multi_batch_device(one, 1, cfg, grid, d_out, ~static_cast<size_t>(0), static_cast<hipStream_t>(stream));  // (one frame: no stride)
}

int mcrt_bake_light_multi_batch_device(mcrt_scene* const* scenes, int n_frames, const mcrt_config* cfg, int grid, const mcrt_bake_planes_multi* d_out,
                                       size_t texel_stride, void* stream) {
    return bake_light_multi_batch_device(scenes, n_frames, cfg, grid, d_out, texel_stride, static_cast<hipStream_t>(stream));
}

int mcrt_scene_texels(mcrt_scene* s, int* n_texels) {
    if (!s || !n_texels) return fail(MCRT_ERR_INVALID, "NULL argument");
    *n_texels = s->n_texels;
    return MCRT_OK;
}

}  // extern "C"
