// host_internal.h — what the host translation units of libmcrt.so share: api.cpp (the C ABI's scene and host-buffer
// entry points), render_enqueue.cpp (a render's launches), device_stores.cpp (what is kept per device or process) and
// probes.cpp.  Not installed; every declaration is hidden, so the library's dynamic symbol table holds none of it.
#pragma once
#include "flatten.h"
#include "kernels.h"
#include "mcrt.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)

namespace mcrt_host {
// set the calling thread's mcrt_last_error() text and return the code (api.cpp, next to the text itself)
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);
}  // namespace mcrt_host
#define HIP_TRY(call)                                               \
    do {                                                            \
        hipError_t e_ = (call);                                     \
        if (e_ != hipSuccess) return mcrt_host::hip_fail(e_, #call); \
    } while (0)

struct DeviceBuffer {
    void* ptr = nullptr;
    size_t bytes = 0;
    hipError_t reserve(size_t need) {
        if (need <= bytes) return hipSuccess;
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
        hipError_t e = hipMalloc(&ptr, need);
        if (e == hipSuccess) bytes = need;
        return e;
    }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { release(); }
};

// A lane renders every n-th tile row of a shard with its own workspace on its own stream.  The
// pipeline of one lane is a chain of dependent kernels whose tails and sparse deeper levels leave
// most of the chip idle; two or three lanes in flight fill those gaps (measured: 1080p 0.53 -> 0.43
// ms, 4K/8 bounces/16 spp 9.6 -> 5.3 ms with three lanes).  Lane 0 runs on the caller's stream,
// the others fork from it and join it through events, so the caller sees ordinary stream order.
constexpr int kMaxLanes = 4;
// what the seeded per-tile mt19937 states in Lane::tile_rng are a function of (tile_renderer.cpp:78: the
// seed is tile.y * width + tile.x) — scene and every other setting do not enter
struct RngKey {
    const void* ptr = nullptr;
    int width = 0, tile_size = 0, first = 0, step = 0, tiles_x = 0, owned_rows = 0;
    int rect[4] = {0, 0, 0, 0};
    int parts = 0, part_twists = 0;  // the engine states at the starts of the streams' parts depend on these too
    bool operator==(const RngKey& o) const {
        return parts == o.parts && part_twists == o.part_twists && ptr == o.ptr && width == o.width && tile_size == o.tile_size && first == o.first && step == o.step && tiles_x == o.tiles_x &&
               owned_rows == o.owned_rows && rect[0] == o.rect[0] && rect[1] == o.rect[1] && rect[2] == o.rect[2] && rect[3] == o.rect[3];
    }
};
struct Lane {
    hipStream_t stream = nullptr;  // owned; unused for lane 0
    hipEvent_t done = nullptr;
    // wavefront workspace, grown on demand (never shrinks; no allocation in the steady state)
    DeviceBuffer tile_rng, tile_draws, scol, end, units, unit_hits, tile_mask, queues[5], texel_refs, targets, cand, lit[2], stack, counters, hit_rng;
    RngKey rng_key;               // which tile seeds tile_rng holds (ptr == nullptr: none)
    bool counters_dirty = false;  // a render's launches failed half way: counters and their base no longer fit (cleared before the next render)
};
template <class LaneT, class F>
void for_each_buffer(LaneT& ln, F f) {  // every workspace buffer of a lane
    for (auto* b : {&ln.tile_rng, &ln.tile_draws, &ln.scol, &ln.end, &ln.units, &ln.unit_hits, &ln.tile_mask, &ln.texel_refs, &ln.targets, &ln.cand,
                    &ln.lit[0], &ln.lit[1], &ln.stack, &ln.counters, &ln.hit_rng}) f(*b);
    for (auto& q : ln.queues) f(q);
}

// One plate of a device (kernels.h) — of a kind: the finished pixels of the gradient background tiles, or every tile's
// draws — and the frame settings its contents are a function of; nothing else enters (RngKey above says the same of the tile
// seeds).  A draw plate's key is its first five fields, the others stay zero.  Entries live in the per-device stores further down.
enum PlateKind { kPlatePixels = 0, kPlateDraws = 1, kPlateKinds = 2 };
struct PlateKey {
    int width, height, tile_size, spp, draws_per_sample, gradient_bg, div_frame;
    float gradient_scale, bg_center[3], bg_edge[3];
};
struct Plate {
    PlateKey key;
    void* ptr = nullptr;    // NULL: the key has been sighted, no plate built (yet)
    size_t bytes = 0;
    int users = 0;          // scene shells (live or pooled) that hold the pointer — in prepared parameters, recorded launch graphs, launches in flight
    int sightings = 0;      // render calls with this key while it had no plate (negative after a failed build: see build_plate)
    unsigned long long last_use = 0;
};

struct mcrt_scene {
    int device = 0;
    int skin_height = 0;  // 64 / 32: a repaintable handle of mcrt_scene_create_skin (the full mesh table of that skin kind); 0: any other
    // LAYOUT: `device` and `skin_height` stay the first two ints of the struct, in this order.  The argument checks that come before
    // any device work read these two members of a handle and nothing else, and the no-device tests (tests/test_layers_abi.py,
    // tests/test_skin_paint_abi.py) hand them zeroed blocks with just these two words set; the assertion below holds the order.
    // `n_texels`, the size of the scene's texel pool, is the third word for the same reason: a bake's stride check reads it
    // (tests/test_bake_abi.py).
    int n_texels = 0;
    // The player model of a repaintable handle (mcrt.h: MCRT_SKIN_CLASSIC 0, MCRT_SKIN_SLIM 1), the fourth word: directly behind
    // the three words the no-device tests already own, so their zeroed blocks stay classic handles.  The batch entries' argument
    // checks do not read it (handles of both models may be mixed); what follows them does.
    int skin_model = 0;
    // Whether a repaintable handle has a cape mesh behind its figure (mcrt.h, "capes"; mcrt_scene_create_skin_cape), the fifth
    // word: zero is "no cape", so the zeroed blocks of the no-device tests stay capeless handles.  The batch entries read it
    // in their argument checks: the handles of one call are all caped or all capeless.
    int has_cape = 0;
    // The handle's extra lights (mcrt.h, "extra lights"; mcrt_scene_set_extra_lights), unused entries zero.  Directly behind the
    // five words above: the passes that refuse a handle with extra lights read the count behind their other argument checks,
    // and the zeroed blocks of the no-device tests then read 0.  Host state only — a render's launches carry a copy as a kernel
    // argument — so a change needs no ordering against renders in flight.  Reset where a pooled shell is reused.
    mcrt::LightSet extra = {};
    uint32_t alpha_words = 0;
    uint32_t n_meshes = 0;
    bool posed = false;  // any mesh with MESH_ROTATED
    // A repaintable handle's view, as mcrt_scene_create_skin or the last mcrt_scene_set_view* gave it: what a NULL pose or look
    // of the next view keeps.  has_pose / has_look false: the builder's own (a NULL argument so far).  Of view_look the light,
    // camera and background fields count; its meshes and textures are NULL.  Reset where a pooled shell is reused.
    bool has_pose = false, has_look = false;
    float view_pose[12] = {};
    mcrt_scene_desc view_look = {};
    std::vector<uint8_t> host_meshes;  // host copy of FlatHeader + FlatMesh[] (screen bounds for workspace planning)
    DeviceBuffer blob;
    // the owner faces of a light bake (kernels.h: BakeFace), uploaded with the blob and kept behind it in the same buffer: a
    // repaint writes texels, alpha predicates and mesh flags only, so the list survives it; a pooled shell gets the next scene's
    size_t bake_faces_offset = 0;
    int bake_n_faces = 0;
    Lane lanes[kMaxLanes];
    int forced_lanes = 0;  // mcrt_scene_set_lanes: 0 = automatic
    int background = MCRT_BACKGROUND_REFERENCE;  // mcrt_scene_set_background
    size_t budget = 0;     // current workspace budget (0 = workspace_budget()); halved when the device is short of memory
    // recorded launch sequences of recent renders (hipGraph), replayed when the parameters repeat
    struct Recorded {
        int n_lanes = 0;
        mcrt::RenderParams p[kMaxLanes];
        mcrt::LightSet lights = {};  // the extra lights the launches carry: part of what a replay must match
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        unsigned long long last_use = 0;
        int sightings = 0;
    };
    static constexpr int kRecorded = 4;
    Recorded recorded[kRecorded];
    unsigned long long use_clock = 0;
    hipStream_t capture_stream = nullptr;
    hipEvent_t fork = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // One handle = one frame in flight: all renders of a handle share its workspace.  `last_done` is recorded
    // at the end of every render; a render enqueued on a different stream than the previous one waits for it.
    hipEvent_t last_done = nullptr;
    std::atomic<hipEvent_t> busy_probe{nullptr};  // = last_done once it exists: what OTHER handles' renders query (device_shared)
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    bool flags_checked = true;  // no render since mcrt_scene_check last read (and cleared) the lanes' overflow words
    // the one-shot host path (mcrt_render & co): frame buffer, streams and events kept with the pooled workspace
    DeviceBuffer frame;                // float4 frame / packed rows / RGBA8 plane of a host-buffer render
    DeviceBuffer pick;                 // mcrt_scene_pick: the pixels' coordinates, then their records (grown on demand)
    hipStream_t main_stream = nullptr;  // the render
    hipStream_t copy_stream = nullptr;  // downloads of finished tile rows, overlapping the render
    std::vector<hipEvent_t> marks;      // event pool of the row-group downloads
    size_t marks_used = 0;
    // pinned host staging for the small transfers of every call (the scene blob up, the lanes' flag words
    // back): no pin / unpin of a few KB of pageable memory per call
    void* staging = nullptr;
    size_t staging_bytes = 0;
    const uint32_t* seed_table = nullptr;  // the device's table of mt19937 seeding results (kernels.h), or NULL
    bool holds_seed_table = false;
    const uint32_t* seed_table_full = nullptr;  // the device's table for every 32-bit seed (ambient occlusion), or NULL
    bool holds_full_table = false, full_table_tried = false;
    const float4* sample_table = nullptr;  // the device's sample table (kernels.h), taken with the plates, or NULL
    bool holds_sample_table = false;
    const void* skin_tables = nullptr;  // a repaintable handle's share of the device's repaint tables (kernels.h: SkinPaintShape)
    DeviceBuffer skin;                  // mcrt_scene_set_skin: the uploaded image
    const void* cape_tables = nullptr;  // a caped handle's share of the device's cape repaint tables (kernels.h: CapePaintShape)
    DeviceBuffer cape;                  // mcrt_scene_set_cape: the uploaded image
    float cape_angle = 0.0f;            // a caped handle's cape angle, as its creation or its last view gave it
    // plates this shell holds a `users` count of, by kind, least recently used first: its recorded launch graphs and its
    // launches in flight may read them, so one is let go of only behind a device synchronisation (acquire_plates)
    std::vector<Plate*> plates[kPlateKinds];
};

static_assert(offsetof(mcrt_scene, device) == 0 && offsetof(mcrt_scene, skin_height) == sizeof(int), "mcrt_scene: device, then skin_height (see the member)");
static_assert(offsetof(mcrt_scene, n_texels) == 2 * sizeof(int), "mcrt_scene: n_texels is the third word (see the member)");
static_assert(offsetof(mcrt_scene, skin_model) == 3 * sizeof(int), "mcrt_scene: skin_model is the fourth word (see the member)");
static_assert(offsetof(mcrt_scene, has_cape) == 4 * sizeof(int), "mcrt_scene: has_cape is the fifth word (see the member)");

namespace mcrt_host {

// Environment knobs.  A knob is read once per process, into a function-local static where it is used — except
// MCRT_WORKSPACE_MB, which workspace_budget() reads at every call.
inline int env_int(const char* name, int fallback) {
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : fallback;
}
inline long long env_ll(const char* name, long long fallback) {
    const char* e = std::getenv(name);
    return e ? std::atoll(e) : fallback;
}
inline bool env_off(const char* name) {  // the kernel paths' development knobs: off when the value begins with '0'
    const char* e = std::getenv(name);
    return e && e[0] == '0';
}

inline bool stream_capturing(hipStream_t stream) {  // the caller records a graph of its own on `stream`
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}
inline bool valid_frame(const mcrt_config* c) { return c->width > 0 && c->height > 0 && c->tile_size > 0; }
inline bool valid_background(int b) { return b == MCRT_BACKGROUND_REFERENCE || b == MCRT_BACKGROUND_TRANSPARENT; }
inline int bad_background() { return fail(MCRT_ERR_INVALID, "background must be MCRT_BACKGROUND_REFERENCE or MCRT_BACKGROUND_TRANSPARENT"); }
// what the passes whose result depends on the light refuse (mcrt.h, "extra lights"), behind their other argument checks
inline int refuse_extra_lights(mcrt_scene* const* scenes, int n) {
    for (int i = 0; i < n; ++i)
        if (scenes[i]->extra.n_extra > 0) return fail(MCRT_ERR_INVALID, "extra lights: beauty render only (mcrt_scene_set_extra_lights with n = 0 takes them off)");
    return MCRT_OK;
}
// a list of extra lights as mcrt_scene_set_extra_lights and mcrt_render_lights take it
inline int check_extra_lights(const mcrt_light_source* lights, int n) {
    if (n < 0 || n > MCRT_MAX_EXTRA_LIGHTS) return fail(MCRT_ERR_INVALID, "a handle takes 0 to 3 extra lights (MCRT_MAX_EXTRA_LIGHTS)");
    if (n > 0 && !lights) return fail(MCRT_ERR_INVALID, "lights is NULL");
    for (int i = 0; i < n; ++i) {
        const mcrt_light_source& l = lights[i];
        bool finite = std::isfinite(l.radius);
        for (const float v : l.position) finite = finite && std::isfinite(v);
        for (const float v : l.color) finite = finite && std::isfinite(v);
        if (!finite) return fail(MCRT_ERR_INVALID, "an extra light's position, radius and colour must be finite");
    }
    return MCRT_OK;
}
inline mcrt::LightSet light_set_of(const mcrt_light_source* lights, int n) {
    mcrt::LightSet set = {};
    set.n_extra = n;
    for (int i = 0; i < n; ++i) set.extra[i] = lights[i];
    return set;
}
inline bool no_plane(const mcrt_layers* l) { return !l->depth && !l->normal && !l->albedo && !l->id; }
inline bool no_plane(const mcrt_ground* g) { return !g->visibility && !g->distance && !g->matte; }
inline bool no_plane(const mcrt_ground_occlusion* g) { return !g->occlusion && !g->matte; }
inline bool no_plane(const mcrt_reflection* r) { return !r->rgba && !r->rgba8 && !r->distance; }
inline bool no_plane(const mcrt_light_planes* l) { return !l->visibility && !l->occlusion && !l->direct; }
// what a light pass refuses of a config (both entry points, before any device work): the truncated engine yields 227 draws — 113
// light samples, 113 AO samples of two draws each — and computeAO divides by ao_samples
inline int check_light_config(const mcrt_config* c, const mcrt_light_planes* out) {
    if (c->soft_shadows && c->shadow_samples > mcrt::kLightMaxSamples)
        return fail(MCRT_ERR_INVALID, "a light pass takes at most 113 shadow samples (the truncated engine's 227 draws)");
    if (out->occlusion && (c->ao_samples < 1 || c->ao_samples > mcrt::kLightMaxSamples))
        return fail(MCRT_ERR_INVALID, "the occlusion plane takes 1 to 113 ao_samples (the truncated engine's 227 draws, two per sample)");
    if (out->occlusion && !std::isfinite(c->ao_radius)) return fail(MCRT_ERR_INVALID, "ao_radius must be finite");
    return MCRT_OK;
}

// what a ground-occlusion pass refuses of a config (every entry point, before any device work): computeAO divides by ao_samples,
// and the truncated engine yields 227 draws, two per sample
inline int check_ground_occlusion_config(const mcrt_config* c) {
    if (c->ao_samples < 1) return fail(MCRT_ERR_INVALID, "a ground-occlusion pass takes at least 1 of ao_samples (the reference divides by it)");
    if (c->ao_samples > mcrt::kLightMaxSamples)
        return fail(MCRT_ERR_INVALID, "a ground-occlusion pass takes at most 113 ao_samples (the truncated engine's 227 draws, two per sample)");
    if (!std::isfinite(c->ao_radius)) return fail(MCRT_ERR_INVALID, "ao_radius must be finite");
    return MCRT_OK;
}

inline bool no_plane(const mcrt_bake_planes* b) { return !b->position && !b->normal && !b->visibility && !b->occlusion && !b->direct; }
// what a light bake refuses of its grid and config (every entry point, before any device work): the light pass's limits
inline int check_bake_config(const mcrt_config* c, int grid, const mcrt_bake_planes* out) {
    if (grid < 1 || grid > mcrt::kBakeMaxGrid) return fail(MCRT_ERR_INVALID, "grid must be 1 to 4 (sub-samples per texel and axis)");
    if (c->soft_shadows && c->shadow_samples > mcrt::kLightMaxSamples)
        return fail(MCRT_ERR_INVALID, "a light bake takes at most 113 shadow samples (the truncated engine's 227 draws)");
    if (out->occlusion && (c->ao_samples < 1 || c->ao_samples > mcrt::kLightMaxSamples))
        return fail(MCRT_ERR_INVALID, "the occlusion plane takes 1 to 113 ao_samples (the truncated engine's 227 draws, two per sample)");
    if (out->occlusion && !std::isfinite(c->ao_radius)) return fail(MCRT_ERR_INVALID, "ao_radius must be finite");
    return MCRT_OK;
}

// the multi-light planes (mcrt.h, "light layers and bake under extra lights"): nothing asked for at all; whether a plane that
// reads the lights is asked for (the `shade_lights` / `bake_shade_lights` kernel runs); the occlusion plane as the single-light
// struct the config checks above read
inline bool light_plane_asked(const mcrt_light_planes_multi* l) {
    bool any = l->combined != nullptr;
    for (int k = 0; k < MCRT_MAX_LIGHTS; ++k) any = any || l->visibility[k] || l->direct[k];
    return any;
}
inline bool light_plane_asked(const mcrt_bake_planes_multi* b) {
    bool any = b->combined != nullptr;
    for (int k = 0; k < MCRT_MAX_LIGHTS; ++k) any = any || b->visibility[k] || b->direct[k];
    return any;
}
inline bool no_plane(const mcrt_light_planes_multi* l) { return !light_plane_asked(l) && !l->occlusion; }
inline bool no_plane(const mcrt_bake_planes_multi* b) { return !light_plane_asked(b) && !b->occlusion && !b->position && !b->normal; }
inline mcrt_light_planes occlusion_alone(const mcrt_light_planes* l) { return mcrt_light_planes{nullptr, l->occlusion, nullptr}; }
inline mcrt_bake_planes occlusion_alone(const mcrt_bake_planes* b) { return mcrt_bake_planes{nullptr, nullptr, nullptr, b->occlusion, nullptr}; }
inline mcrt_light_planes occlusion_alone(const mcrt_light_planes_multi* l) { return mcrt_light_planes{nullptr, l->occlusion, nullptr}; }
inline mcrt_bake_planes occlusion_alone(const mcrt_bake_planes_multi* b) { return mcrt_bake_planes{nullptr, nullptr, nullptr, b->occlusion, nullptr}; }

// what every studio-shot entry point refuses of the shot itself (before any device work)
inline int check_shot(const mcrt_shot* s) {
    if (s->page != MCRT_PAGE_COLOR && s->page != MCRT_PAGE_REFERENCE) return fail(MCRT_ERR_INVALID, "page must be MCRT_PAGE_COLOR or MCRT_PAGE_REFERENCE");
    if (!(s->shadow_strength >= 0.0f && s->shadow_strength <= 1.0f)) return fail(MCRT_ERR_INVALID, "shadow_strength must lie in [0, 1]");
    if (!(s->reflectivity >= 0.0f && s->reflectivity <= 1.0f)) return fail(MCRT_ERR_INVALID, "reflectivity must lie in [0, 1]");
    if (!(s->reflection_fade >= 0.0f) || !std::isfinite(s->reflection_fade)) return fail(MCRT_ERR_INVALID, "reflection_fade must be finite and >= 0");
    for (const float c : s->page_color)
        if (!std::isfinite(c)) return fail(MCRT_ERR_INVALID, "page_color must be finite");
    return MCRT_OK;
}
// the strength of the floor-occlusion term (the _occ entry points)
inline int check_floor_occlusion(float o) {
    if (!(o >= 0.0f && o <= 1.0f)) return fail(MCRT_ERR_INVALID, "floor_occlusion must lie in [0, 1]");
    return MCRT_OK;
}
// What a shot entry point asks for, as the shot's host paths pass it on: the caller's shot (NULL is refused where the entries
// refuse it), the strength of the floor-occlusion term (0 from the plain entries) and what the _ex entries add — the shadow's
// colour, the bounds (device memory behind the device forms, host memory behind the host forms) and the PNG's crop.  `ex`: an
// _ex entry called; the page may then be MCRT_PAGE_TRANSPARENT, and the checks and their messages are that family's.
struct ShotSpec {
    const mcrt_shot* shot = nullptr;
    float floor_occlusion = 0.0f;
    float shadow_color[3] = {0.0f, 0.0f, 0.0f};
    int32_t (*bounds)[4] = nullptr;
    bool crop = false;  // mcrt_render_shot_png_ex's: like the bounds, only with the transparent page
    bool ex = false;
};
inline ShotSpec shot_spec(const mcrt_shot* shot, float floor_occlusion) {
    ShotSpec spec;
    spec.shot = shot, spec.floor_occlusion = floor_occlusion;
    return spec;
}
inline ShotSpec shot_spec_ex(const mcrt_shot_ex* shot, int32_t (*bounds)[4], bool crop = false) {  // (a NULL shot stays NULL)
    ShotSpec spec;
    if (shot) {
        spec.shot = &shot->shot, spec.floor_occlusion = shot->floor_occlusion;
        std::memcpy(spec.shadow_color, shot->shadow_color, sizeof spec.shadow_color);
    }
    spec.bounds = bounds, spec.crop = crop, spec.ex = true;
    return spec;
}
// what the _ex entries refuse of the shot: check_shot's list with the third page, then the colour and what needs the transparent page
inline int check_shot_ex(const mcrt_shot* s, const ShotSpec& ex) {
    if (s->page < MCRT_PAGE_COLOR || s->page > MCRT_PAGE_TRANSPARENT)
        return fail(MCRT_ERR_INVALID, "page must be MCRT_PAGE_COLOR, MCRT_PAGE_REFERENCE or MCRT_PAGE_TRANSPARENT");
    mcrt_shot on_a_page = *s;
    if (s->page == MCRT_PAGE_TRANSPARENT) on_a_page.page = MCRT_PAGE_COLOR;
    if (const int rc = check_shot(&on_a_page); rc != MCRT_OK) return rc;
    for (const float c : ex.shadow_color)
        if (!std::isfinite(c)) return fail(MCRT_ERR_INVALID, "shadow_color must be finite");
    if (s->page != MCRT_PAGE_TRANSPARENT && (ex.bounds || ex.crop)) return fail(MCRT_ERR_INVALID, "bounds and crop come with MCRT_PAGE_TRANSPARENT only");
    return MCRT_OK;
}
inline int check_shot(const ShotSpec& spec) { return spec.ex ? check_shot_ex(spec.shot, spec) : check_shot(spec.shot); }
// and of the config of a shot that renders: the render's limit, and the limits of the passes the shot runs
int validate_config(const mcrt_config* cfg);
inline int check_shot_config(const mcrt_config* c, const mcrt_shot* s, float floor_occlusion = 0.0f) {
    if (validate_config(c) != MCRT_OK) return MCRT_ERR_INVALID;
    const bool ground = s->shadow_strength > 0.0f, mirror = s->reflectivity > 0.0f;
    if ((ground || mirror) && c->soft_shadows && c->shadow_samples > mcrt::kGroundMaxSamples)
        return fail(MCRT_ERR_INVALID, "a shot with a shadow or a reflection takes at most 113 shadow samples (the truncated engine's 227 draws)");
    if (mirror && c->max_bounces > mcrt::kReflectMaxBounces)
        return fail(MCRT_ERR_INVALID, "a shot with a reflection takes at most 8 bounces (the reflection pass's per-lane colour stack)");
    if (floor_occlusion > 0.0f) return check_ground_occlusion_config(c);
    return MCRT_OK;
}
inline bool shot_frame_too_large(const mcrt_config* c) { return static_cast<long long>(c->width) * c->height >= (1ll << 31); }
// The scratch of a shot that renders (include/mcrt.h): the planes it needs, each for n frames and each on a 16-byte boundary.
// Offsets of the absent planes are SIZE_MAX.  The floor-occlusion plane lies behind the others, so they keep their offsets.
struct ShotScratch {
    size_t figure = 0, reflection = SIZE_MAX, visibility = SIZE_MAX, distance = SIZE_MAX, occlusion = SIZE_MAX, bytes = 0;
};
inline ShotScratch shot_scratch(const mcrt_config* c, const mcrt_shot* s, int n, float floor_occlusion = 0.0f) {
    ShotScratch l;
    const size_t px = static_cast<size_t>(c->width) * static_cast<size_t>(c->height) * static_cast<size_t>(n);
    auto place = [&](size_t px_bytes) {
        const size_t at = l.bytes;
        l.bytes += (px * px_bytes + 15) & ~static_cast<size_t>(15);
        return at;
    };
    l.figure = place(16);
    if (s->reflectivity > 0.0f) l.reflection = place(16);
    if (s->shadow_strength > 0.0f) l.visibility = place(4);
    if (s->reflectivity > 0.0f && s->reflection_fade > 0.0f) l.distance = place(4);
    if (floor_occlusion > 0.0f) l.occlusion = place(4);
    return l;
}

// what the calling thread's last mcrt_render_batch* call did (mcrt_last_batch_info; thread-local in api.cpp, like the error text)
struct BatchInfo {
    int frames = 0, sequences = 0;
};
BatchInfo& last_batch();

// ---- device_stores.cpp: per device or per process, each store under a mutex of its own (none is held while another is taken)
size_t device_total_memory(int device);
// every shell of the process is on the live list from its creation to destroy_scene_now
void register_live(mcrt_scene* s);
bool device_shared(const mcrt_scene* s);  // another handle's frame is in flight on s's device right now
// the device's table of mt19937 seeding results for the seeds of a frame's tiles and hits, or nullptr; one `users` count per call
const uint32_t* acquire_seed_table(int device);
// the first ambient-occlusion render of a shell takes the device's table for every 32-bit seed (never built while `stream` is capturing)
void ensure_full_seed_table(mcrt_scene* s, hipStream_t stream);
// a shell that does not hold the device's table for every seed takes it where it is ALREADY built (a light pass's occlusion
// plane: it never builds the table); no launch, no wait
void share_full_seed_table(mcrt_scene* s);
// the device's background plate and draw plate for the frame prepared as p[0] — each or nullptr, both kinds under one sighting
// rule in this one call — into bg_plate and draw_plate of p[0..n) (the lanes of one render read the same plates); and, by the
// same rule in the same call, the device's sample table into sample_table
void acquire_plates(mcrt_scene* s, mcrt::RenderParams* p, int n, bool capturing, bool count_sighting);
// the rows of `seeds` (kSampleRow float4 each, seeds inside the window) of the device's sample table to the host, for the probe;
// the table is built if the device has none yet (whatever the sighting count); false where it cannot be
bool copy_sample_rows(int device, const int32_t* seeds, int n, float* out);
// the words of `seeds` of the device's window table (MCRT_TABLE_WINDOW: seeds inside the window) or its table of all seeds
// (MCRT_TABLE_FULL) to the host, for the probe; the table is built if the device has none yet, and the call's count let go of
// afterwards; false where there is no table (the knob, no room) or a seed lies outside the window
bool copy_seed_words(int device, int which, const uint32_t* seeds, int n, uint32_t* out);
// The device's repaint tables of a skin kind (64 / 32) — the 256 floats u8 / 255.0f, then per pool texel the mesh and the skin
// pixel it is cut from (kernels.h: SkinPaintShape) — built at the kind's first repaintable handle on the device, one `users`
// count per handle that holds them, freed by mcrt_trim() when nobody does.  nullptr: the allocation or the upload failed.
// the kinds of the kind-keyed stores: 0 a classic 64x64 skin, 1 a 64x32 one, 2 a slim 64x64 one
constexpr int kSkinKinds = 3;
inline int skin_kind_index(int skin_height, int model) { return skin_height == 32 ? 1 : (model == 1 ? 2 : 0); }
const void* acquire_skin_tables(int device, int skin_height, int model);
void release_skin_tables(int device, int skin_height, int model);
// and the cape's (kernels.h: CapePaintShape), one per device, held by caped handles in the same way
const void* acquire_cape_tables(int device);
void release_cape_tables(int device);
size_t pool_limit(int device);
bool pool_scene(mcrt_scene* s);             // false: not kept, the caller destroys it
mcrt_scene* take_pooled_scene(int device);  // device < 0: any
void destroy_scene_now(mcrt_scene* s);
// A parameter table of a batched launch set, in a slot of the device's ring.  upload_table() takes the slot, waits until
// the launches that last read it have finished, and enqueues the rows' copy on `stream`; the caller launches what reads
// `dev`, then commit()s.  The slot is given back when the guard goes, committed or not.
struct TableSlot;
struct TableUpload {
    TableSlot* slot = nullptr;
    const void* dev = nullptr;        // the rows on the device
    hipError_t status = hipSuccess;   // of the rows' asynchronous copy: reported by the caller, with its launches
    hipError_t commit(hipStream_t stream);  // behind the launches that read the table: records the slot's event
    TableUpload() = default;
    TableUpload(const TableUpload&) = delete;
    TableUpload& operator=(const TableUpload&) = delete;
    ~TableUpload();
};
int upload_table(int device, const void* rows, size_t bytes, hipStream_t stream, TableUpload& up);

// ---- render_enqueue.cpp
size_t workspace_budget(int device);
int validate_config(const mcrt_config* cfg);
// Tile rows that become final together, for a caller that downloads rows while the rest still renders.
struct RowGroup {
    std::vector<hipEvent_t> wait;  // recorded events after which the rows are complete in device memory
    std::vector<int> rows;         // tile-row indices in the frame
};
hipEvent_t next_mark(mcrt_scene* s);  // an event of the shell's pool (nullptr: creation failed)
// enqueue one render of the shard (first, step) on `stream`.  groups != nullptr (one-shot host path): the launches also record events
// that tell when which tile rows are final, *groups lists them in completion order (direct launches: the events are this call's own).
int enqueue_render(mcrt_scene* s, const mcrt_config* cfg, int first, int step, int layout, float* d_out, uint8_t* d_out8, hipStream_t stream,
                   bool may_record = true, std::vector<RowGroup>* groups = nullptr, const mcrt_tile* rect = nullptr);
int render_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, float* d_f32, uint8_t* d_u8, size_t stride, hipStream_t stream);
int render_layers_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, const mcrt_layers* d_out, size_t stride, hipStream_t stream);
int render_ground_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, const float* ground_y, const mcrt_ground* d_out, size_t stride,
                               hipStream_t stream);
int render_ground_occlusion_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, const float* ground_y, const mcrt_ground_occlusion* d_out,
                                         size_t stride, hipStream_t stream);
int render_reflection_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, const float* ground_y, const mcrt_reflection* d_out,
                                   size_t stride, hipStream_t stream);
int render_light_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, const mcrt_light_planes* d_out, size_t stride, hipStream_t stream);
int bake_light_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, int grid, const mcrt_bake_planes* d_out, size_t stride, hipStream_t stream);
// the same two passes with planes per light, for handles with extra lights too (mcrt_render_light_multi_device, mcrt_bake_light_multi_device & co)
int render_light_multi_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, const mcrt_light_planes_multi* d_out, size_t stride,
                                    hipStream_t stream);
int bake_light_multi_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, int grid, const mcrt_bake_planes_multi* d_out, size_t stride,
                                  hipStream_t stream);
// the studio shot's blend on the caller's planes (mcrt_composite_shot_batch_device[_occ]), and render + ground + reflection +
// ground occlusion + blend on `stream` in order with the planes in the caller's scratch (mcrt_render_shot_batch_device[_occ]);
// the entries without the floor-occlusion term pass a spec with floor_occlusion = 0 and no plane; spec.bounds: device memory
int composite_shot_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, const ShotSpec& spec, const mcrt_shot_inputs* d_in,
                                const float* d_occlusion, size_t in_stride, float* d_f32, uint8_t* d_u8, size_t out_stride, hipStream_t stream);
int render_shot_batch_device(mcrt_scene* const* scenes, int n, const mcrt_config* cfg, const ShotSpec& spec, const float* ground_y, void* d_scratch,
                             size_t scratch_bytes, float* d_f32, uint8_t* d_u8, size_t stride, hipStream_t stream);
// repaints the n repaintable handles from the skin images at d_skins + i * stride_bytes (mcrt_scene_set_skins_batch_device)
int set_skins_batch_device(mcrt_scene* const* scenes, int n, const uint8_t* d_skins, size_t stride_bytes, hipStream_t stream);
// gives the n repaintable handles the views (poses[i], looks[i]); NULL poses, looks or looks[i]: the handle's own
// (mcrt_scene_set_views_batch_device)
int set_views_batch_device(mcrt_scene* const* scenes, int n, const float (*poses)[12], const mcrt_scene_desc* const* looks, hipStream_t stream);
// the same with one cape angle per caped handle, cape_angles NULL: kept (mcrt_scene_set_views_cape_batch_device)
int set_views_cape_batch_device(mcrt_scene* const* scenes, int n, const float (*poses)[12], const mcrt_scene_desc* const* looks, const float* cape_angles,
                                hipStream_t stream);
// repaints the capes of the n caped handles from the 64x32 images at d_capes + i * stride_bytes (mcrt_scene_set_capes_batch_device)
int set_capes_batch_device(mcrt_scene* const* scenes, int n, const uint8_t* d_capes, size_t stride_bytes, hipStream_t stream);

// ---- api.cpp
// the light, camera and background fields of `look` into `desc` (what mcrt_scene_create_skin reads of a look)
void apply_look(mcrt_scene_desc* desc, const mcrt_scene_desc* look);
// The prefix [FlatHeader][FlatMesh x n] of the blob of the kind's white figure at pose / look (NULL: the builder's own), with
// MESH_OPAQUE on every mesh as that figure has it.  No device work.
int skin_view_table(int skin_height, int model, const float pose[12], const mcrt_scene_desc* look, std::vector<uint8_t>& table);
// the same for the caped figure (mcrt.h, "capes"): one more mesh, the cape at cape_angle, also with MESH_OPAQUE
int skin_view_table_cape(int skin_height, int model, const float pose[12], const mcrt_scene_desc* look, float cape_angle, std::vector<uint8_t>& table);
inline bool cape_angle_ok(float a) { return a >= 0.0f && a <= 90.0f; }  // (false for NaN)

}  // namespace mcrt_host

#pragma GCC visibility pop
