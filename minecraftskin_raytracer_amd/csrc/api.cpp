// api.cpp — C-ABI implementation of include/mcrt.h, host side: scenes, the host-buffer entry points and the calling
// thread's error text and timings.  The launches of a render are in render_enqueue.cpp, what is kept per device in
// device_stores.cpp, the probes in probes.cpp, the planning of the launches in render_plan.cpp, the kernels in
// render_kernels.hip, pass_kernels.hip and util_kernels.hip.
//
// There is deliberately no CPU fallback anywhere in the library: every render / probe entry point
// needs a HIP device and fails with MCRT_ERR_NO_DEVICE / MCRT_ERR_HIP otherwise.
#include "host_internal.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <utility>

using namespace mcrt;
using namespace mcrt_host;

namespace {
thread_local std::string g_err;
thread_local mcrt_timings g_timings = {0, 0, 0, 0, 0};
thread_local BatchInfo g_batch;

double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}
}  // namespace

namespace mcrt_host {
BatchInfo& last_batch() { return g_batch; }
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int hip_fail(hipError_t e, const char* what) {
    return fail(e == hipErrorNoDevice || e == hipErrorInvalidDevice ? MCRT_ERR_NO_DEVICE : MCRT_ERR_HIP,
                std::string(what) + ": " + hipGetErrorString(e));
}
}  // namespace mcrt_host
// error hook for the library's other translation units (png_writer.cpp, scene_builder.cpp)
__attribute__((visibility("hidden"))) int mcrt_detail_fail(int code, const char* msg) { return fail(code, msg ? msg : ""); }

extern "C" {

int mcrt_abi_version(void) { return MCRT_ABI_VERSION; }

int mcrt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* mcrt_last_error(void) { return g_err.c_str(); }

void mcrt_config_init(mcrt_config* c) {  // raytracer.h:10-38
    if (!c) return;
    c->width = 256;
    c->height = 256;
    c->max_bounces = 3;
    c->samples_per_pixel = 1;
    c->tile_size = 32;
    c->thread_count = 0;
    c->soft_shadows = 1;
    c->shadow_samples = 8;
    c->ao_enabled = 0;
    c->ao_samples = 8;
    c->ao_radius = 3.0f;
    c->ao_intensity = 0.5f;
    c->dof_enabled = 0;
    c->aperture = 0.5f;
    c->focus_distance = 0.0f;
    c->gradient_bg = 1;
    c->gradient_scale = 1.0f;
    const float center[4] = {0.91f, 0.89f, 0.86f, 1.0f}, edge[4] = {0.56f, 0.63f, 0.71f, 1.0f};
    std::memcpy(c->bg_center, center, 16);
    std::memcpy(c->bg_edge, edge, 16);
}

int mcrt_generate_tiles(int w, int h, int ts, mcrt_tile* tiles, int capacity) {  // tile_renderer.cpp:18-39
    if (w <= 0 || h <= 0 || ts <= 0) return 0;
    int cols = (w + ts - 1) / ts, rows = (h + ts - 1) / ts;
    int n = 0;
    for (int ty = 0; ty < rows; ++ty)
        for (int tx = 0; tx < cols; ++tx, ++n) {
            if (!tiles || n >= capacity) continue;
            mcrt_tile& t = tiles[n];
            t.x = tx * ts;
            t.y = ty * ts;
            t.width = ts < w - t.x ? ts : w - t.x;
            t.height = ts < h - t.y ? ts : h - t.y;
        }
    return n;
}

size_t mcrt_scene_flatten(const mcrt_scene_desc* desc, void* blob, size_t capacity) {
    std::vector<uint8_t> b;
    std::string err;
    if (!flatten_scene(desc, b, err)) {
        g_err = err;
        return 0;
    }
    if (blob && capacity) std::memcpy(blob, b.data(), b.size() < capacity ? b.size() : capacity);
    return b.size();
}

}  // extern "C"
namespace {
// uploads an already flattened scene to `device` (a pooled shell with its workspace when one is idle)
int create_scene_from_blob(const std::vector<uint8_t>& b, int device, mcrt_scene** out) {
    *out = nullptr;
    int n = mcrt_device_count();
    if (n <= 0) return fail(MCRT_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= n) return fail(MCRT_ERR_NO_DEVICE, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    mcrt_scene* s = take_pooled_scene(device);  // an idle shell with its workspace, or nullptr
    if (!s) {
        s = new mcrt_scene();
        s->device = device;
        register_live(s);
    }
    s->forced_lanes = 0;
    s->background = MCRT_BACKGROUND_REFERENCE;
    s->extra = mcrt::LightSet{};  // a pooled shell's extra lights go with its previous scene
    if (s->skin_tables) release_skin_tables(device, s->skin_height, s->skin_model);  // a pooled shell that was a repaintable handle
    s->skin_tables = nullptr;
    s->skin_height = 0;
    s->skin_model = MCRT_SKIN_CLASSIC;
    if (s->cape_tables) release_cape_tables(device);  // a pooled shell that was a caped handle
    s->cape_tables = nullptr;
    s->has_cape = 0;
    s->cape_angle = 0.0f;
    s->has_pose = s->has_look = false;  // (mcrt_scene_create_skin notes its own)
    s->budget = 0;  // a budget halved under memory pressure is not inherited
    s->have_last = false;  // a pooled shell was synchronised when its previous owner let go of it
    s->last_stream = nullptr;
    s->marks_used = 0;
    if (!s->holds_seed_table) {
        s->seed_table = acquire_seed_table(device);
        s->holds_seed_table = s->seed_table != nullptr;
    }
    const FlatHeader* fh = reinterpret_cast<const FlatHeader*>(b.data());
    const FlatMesh* fm = reinterpret_cast<const FlatMesh*>(b.data() + fh->mesh_offset);
    s->alpha_words = fh->alpha_words;
    s->n_meshes = fh->n_meshes;
    s->posed = false;
    for (uint32_t i = 0; i < fh->n_meshes; ++i) s->posed = s->posed || (fm[i].flags & MESH_ROTATED) != 0;
    s->host_meshes.assign(b.begin(), b.begin() + fh->mesh_offset + sizeof(FlatMesh) * fh->n_meshes);
    // the owner faces of a light bake travel with the blob, 16-byte aligned behind it
    std::vector<BakeFace> owners;
    bake_owner_faces(b.data(), owners);
    s->n_texels = static_cast<int>(fh->n_texels);
    s->bake_faces_offset = (b.size() + 15) & ~static_cast<size_t>(15);
    s->bake_n_faces = static_cast<int>(owners.size());
    const size_t upload = s->bake_faces_offset + owners.size() * sizeof(BakeFace);
    hipError_t e = s->blob.reserve(upload);
    const size_t staging_need = upload + 64;  // the blob and the owner faces, then the lanes' flag words
    if (e == hipSuccess && s->staging_bytes < staging_need) {
        if (s->staging) (void)hipHostFree(s->staging);
        s->staging = nullptr;
        s->staging_bytes = 0;
        e = hipHostMalloc(&s->staging, staging_need + (staging_need >> 2), hipHostMallocDefault);
        if (e == hipSuccess) s->staging_bytes = staging_need + (staging_need >> 2);
    }
    if (e == hipSuccess) {
        std::memcpy(s->staging, b.data(), b.size());
        std::memset(static_cast<char*>(s->staging) + b.size(), 0, s->bake_faces_offset - b.size());
        if (!owners.empty()) std::memcpy(static_cast<char*>(s->staging) + s->bake_faces_offset, owners.data(), owners.size() * sizeof(BakeFace));
        e = hipMemcpy(s->blob.ptr, s->staging, upload, hipMemcpyHostToDevice);
    }
    for (int i = 0; i < 4 && e == hipSuccess; ++i)
        if (!s->ev[i]) e = hipEventCreate(&s->ev[i]);
    if (e != hipSuccess) {
        destroy_scene_now(s);
        return hip_fail(e, "scene upload");
    }
    *out = s;
    return MCRT_OK;
}

// what a NULL pose or look of the handle's next view keeps (host_internal.h: view_pose, view_look)
void remember_view(mcrt_scene* s, const float pose[12], const mcrt_scene_desc* look) {
    s->has_pose = pose != nullptr;
    if (pose) std::memcpy(s->view_pose, pose, sizeof s->view_pose);
    s->has_look = look != nullptr;
    if (look) apply_look(&s->view_look, look);  // (the other fields stay zero)
}
}  // namespace

extern "C" mcrt_scene_desc* mcrt_detail_white_figure(int skin_height, int model, const float pose[12]);  // scene_builder.cpp
extern "C" mcrt_scene_desc* mcrt_detail_white_figure_cape(int skin_height, int model, const float pose[12], float cape_angle, int cape_alpha);

namespace mcrt_host {
void apply_look(mcrt_scene_desc* desc, const mcrt_scene_desc* look) {
    std::memcpy(desc->light_position, look->light_position, sizeof desc->light_position);
    std::memcpy(desc->light_color, look->light_color, sizeof desc->light_color);
    desc->light_intensity = look->light_intensity;
    desc->light_radius = look->light_radius;
    std::memcpy(desc->camera_position, look->camera_position, sizeof desc->camera_position);
    std::memcpy(desc->camera_target, look->camera_target, sizeof desc->camera_target);
    std::memcpy(desc->camera_up, look->camera_up, sizeof desc->camera_up);
    desc->camera_fov = look->camera_fov;
    std::memcpy(desc->background_color, look->background_color, sizeof desc->background_color);
}

int skin_view_table(int skin_height, int model, const float pose[12], const mcrt_scene_desc* look, std::vector<uint8_t>& table) {
    if (skin_height != 64 && skin_height != 32) return fail(MCRT_ERR_INVALID, "skin_height must be 64 or 32");
    if (model != MCRT_SKIN_CLASSIC && !(model == MCRT_SKIN_SLIM && skin_height == 64))
        return fail(MCRT_ERR_INVALID, "model must be MCRT_SKIN_CLASSIC, or MCRT_SKIN_SLIM with a 64x64 skin");
    mcrt_scene_desc* desc = mcrt_detail_white_figure(skin_height, model, pose);
    if (look) apply_look(desc, look);
    std::string err;
    const bool flat = flatten_view_table(desc, table, err);
    mcrt_scene_desc_free(desc);
    if (!flat) return fail(MCRT_ERR_INVALID, err);
    // the white figure's own MESH_OPAQUE bits: every texel of an all-(255,255,255,255) skin is opaque
    const FlatHeader* h = reinterpret_cast<const FlatHeader*>(table.data());
    FlatMesh* fm = reinterpret_cast<FlatMesh*>(table.data() + h->mesh_offset);
    for (uint32_t i = 0; i < h->n_meshes; ++i) fm[i].flags |= MESH_OPAQUE;
    return MCRT_OK;
}

int skin_view_table_cape(int skin_height, int model, const float pose[12], const mcrt_scene_desc* look, float cape_angle, std::vector<uint8_t>& table) {
    if (skin_height != 64 && skin_height != 32) return fail(MCRT_ERR_INVALID, "skin_height must be 64 or 32");
    if (model != MCRT_SKIN_CLASSIC && !(model == MCRT_SKIN_SLIM && skin_height == 64))
        return fail(MCRT_ERR_INVALID, "model must be MCRT_SKIN_CLASSIC, or MCRT_SKIN_SLIM with a 64x64 skin");
    if (!cape_angle_ok(cape_angle)) return fail(MCRT_ERR_INVALID, "cape_angle must be within 0 .. 90 degrees");
    mcrt_scene_desc* desc = mcrt_detail_white_figure_cape(skin_height, model, pose, cape_angle, 255);
    if (look) apply_look(desc, look);
    std::string err;
    const bool flat = flatten_view_table(desc, table, err);
    mcrt_scene_desc_free(desc);
    if (!flat) return fail(MCRT_ERR_INVALID, err);
    // the white figure's and the white cape's own MESH_OPAQUE bits
    const FlatHeader* h = reinterpret_cast<const FlatHeader*>(table.data());
    FlatMesh* fm = reinterpret_cast<FlatMesh*>(table.data() + h->mesh_offset);
    for (uint32_t i = 0; i < h->n_meshes; ++i) fm[i].flags |= MESH_OPAQUE;
    return MCRT_OK;
}
}  // namespace mcrt_host

extern "C" {

int mcrt_scene_create(const mcrt_scene_desc* desc, int device, mcrt_scene** out) {
    if (!out) return fail(MCRT_ERR_INVALID, "out is NULL");
    *out = nullptr;
    std::vector<uint8_t> b;
    std::string err;
    if (!flatten_scene(desc, b, err)) return fail(MCRT_ERR_INVALID, err);
    return create_scene_from_blob(b, device, out);
}

int mcrt_scene_create_skin(int skin_height, const float pose[12], const mcrt_scene_desc* look, int device, mcrt_scene** out) {
    return mcrt_scene_create_skin_model(skin_height, MCRT_SKIN_CLASSIC, pose, look, device, out);
}

int mcrt_scene_create_skin_model(int skin_height, int model, const float pose[12], const mcrt_scene_desc* look, int device, mcrt_scene** out) {
    if (!out) return fail(MCRT_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (skin_height != 64 && skin_height != 32) return fail(MCRT_ERR_INVALID, "skin_height must be 64 or 32");
    if (model != MCRT_SKIN_CLASSIC && !(model == MCRT_SKIN_SLIM && skin_height == 64))
        return fail(MCRT_ERR_INVALID, "model must be MCRT_SKIN_CLASSIC, or MCRT_SKIN_SLIM with a 64x64 skin");
    // the builder's figure of an all-opaque white skin: no outer part is dropped, so the mesh table is the full one of
    // mcrt_skin_texel[_model] (12 meshes, or 7) and the pool holds a slot for every texel a skin of this kind can show
    const std::vector<uint8_t> white(static_cast<size_t>(64) * static_cast<size_t>(skin_height) * 4, 255);
    mcrt_scene_desc* desc = nullptr;
    if (mcrt_build_skin_scene_model(white.data(), 64, skin_height, model, pose, &desc) != MCRT_OK || !desc) return fail(MCRT_ERR_INVALID, "the scene builder failed");
    if (look) apply_look(desc, look);
    std::vector<uint8_t> b;
    std::string err;
    const bool flat = flatten_scene(desc, b, err);
    mcrt_scene_desc_free(desc);
    if (!flat) return fail(MCRT_ERR_INVALID, err);
    mcrt_scene* s = nullptr;
    if (const int rc = create_scene_from_blob(b, device, &s); rc != MCRT_OK) return rc;
    s->skin_model = model;  // (before the tables: a shell's release names the store by its own height and model)
    s->skin_tables = acquire_skin_tables(device, skin_height, model);
    if (!s->skin_tables) {
        s->skin_model = MCRT_SKIN_CLASSIC;
        mcrt_scene_destroy(s);
        return fail(MCRT_ERR_HIP, "the device's repaint tables could not be built");
    }
    s->skin_height = skin_height;
    remember_view(s, pose, look);
    *out = s;
    return MCRT_OK;
}

int mcrt_scene_create_skin_cape(int skin_height, int model, const float pose[12], const mcrt_scene_desc* look, float cape_angle, int device, mcrt_scene** out) {
    if (!out) return fail(MCRT_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (skin_height != 64 && skin_height != 32) return fail(MCRT_ERR_INVALID, "skin_height must be 64 or 32");
    if (model != MCRT_SKIN_CLASSIC && !(model == MCRT_SKIN_SLIM && skin_height == 64))
        return fail(MCRT_ERR_INVALID, "model must be MCRT_SKIN_CLASSIC, or MCRT_SKIN_SLIM with a 64x64 skin");
    if (!cape_angle_ok(cape_angle)) return fail(MCRT_ERR_INVALID, "cape_angle must be within 0 .. 90 degrees");
    // the white figure with a cape mesh that is kept although every texel of it is transparent: the full table of 13 or 8
    // meshes, the cape's texels zero, its predicate words "alpha == 0" and its MESH_OPAQUE clear — all the flattener's own
    mcrt_scene_desc* desc = mcrt_detail_white_figure_cape(skin_height, model, pose, cape_angle, 0);
    if (!desc) return fail(MCRT_ERR_INVALID, "the scene builder failed");
    if (look) apply_look(desc, look);
    std::vector<uint8_t> b;
    std::string err;
    const bool flat = flatten_scene(desc, b, err);
    mcrt_scene_desc_free(desc);
    if (!flat) return fail(MCRT_ERR_INVALID, err);
    mcrt_scene* s = nullptr;
    if (const int rc = create_scene_from_blob(b, device, &s); rc != MCRT_OK) return rc;
    s->skin_model = model;  // (before the tables: a shell's release names the store by its own height and model)
    s->skin_tables = acquire_skin_tables(device, skin_height, model);
    s->cape_tables = s->skin_tables ? acquire_cape_tables(device) : nullptr;
    if (!s->skin_tables || !s->cape_tables) {
        if (s->skin_tables) release_skin_tables(device, skin_height, model);
        s->skin_tables = nullptr;
        s->skin_model = MCRT_SKIN_CLASSIC;
        mcrt_scene_destroy(s);
        return fail(MCRT_ERR_HIP, "the device's repaint tables could not be built");
    }
    s->skin_height = skin_height;
    s->has_cape = 1;
    s->cape_angle = cape_angle;
    remember_view(s, pose, look);
    *out = s;
    return MCRT_OK;
}

int mcrt_skin_view_table_cape(int skin_height, int model, const float pose[12], const mcrt_scene_desc* look, float cape_angle, void* out, size_t capacity) {
    std::vector<uint8_t> t;
    if (skin_view_table_cape(skin_height, model, pose, look, cape_angle, t) != MCRT_OK) return 0;
    if (out && capacity) std::memcpy(out, t.data(), t.size() < capacity ? t.size() : capacity);
    return static_cast<int>(t.size());
}

int mcrt_skin_view_table(int skin_height, const float pose[12], const mcrt_scene_desc* look, void* out, size_t capacity) {
    return mcrt_skin_view_table_model(skin_height, MCRT_SKIN_CLASSIC, pose, look, out, capacity);
}

int mcrt_skin_view_table_model(int skin_height, int model, const float pose[12], const mcrt_scene_desc* look, void* out, size_t capacity) {
    std::vector<uint8_t> t;
    if (skin_view_table(skin_height, model, pose, look, t) != MCRT_OK) return 0;
    if (out && capacity) std::memcpy(out, t.data(), t.size() < capacity ? t.size() : capacity);
    return static_cast<int>(t.size());
}

void mcrt_scene_destroy(mcrt_scene* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();  // renders of this scene may still be running on the caller's streams
    if (!s->flags_checked) (void)mcrt_scene_check(s);  // reads and clears the lanes' sticky overflow words: the next owner of the workspace starts clean
    // A modest workspace is kept for the next scene on this device (one idle shell per device): a fresh
    // hipMalloc of the lanes' buffers costs milliseconds per render call of the one-shot API
    // (TileRenderer::render), tens of GB for large frames take far longer.  mcrt_trim() lets go of it.
    if (pool_scene(s)) return;
    destroy_scene_now(s);
}

int mcrt_scene_check(mcrt_scene* s) {
    if (!s) return fail(MCRT_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    bool flagged = false;
    uint32_t* flags = reinterpret_cast<uint32_t*>(static_cast<char*>(s->staging) + (s->staging_bytes - 64));  // pinned
    int li = 0;
    for (Lane& ln : s->lanes) {
        ++li;
        if (!ln.counters.ptr) continue;
        uint32_t* word = static_cast<uint32_t*>(ln.counters.ptr) + (kCounterWords - 1);
        uint32_t local = 0;
        uint32_t* dst = s->staging ? &flags[li - 1] : &local;
        HIP_TRY(hipMemcpy(dst, word, 4, hipMemcpyDeviceToHost));
        const uint32_t flag = *dst;
        if (flag) {  // reported once: the word is cleared so that later renders (and the next owner of a pooled workspace) start clean
            flagged = true;
            HIP_TRY(hipMemset(word, 0, 4));
        }
    }
    s->flags_checked = true;
    if (flagged) return fail(MCRT_ERR_HIP, "internal error: more tiles were touched than the workspace was planned for");
    return MCRT_OK;
}

int mcrt_scene_set_lanes(mcrt_scene* s, int lanes) {
    if (!s || lanes < 0) return fail(MCRT_ERR_INVALID, "bad argument");
    s->forced_lanes = lanes;
    return MCRT_OK;
}

int mcrt_scene_set_background(mcrt_scene* s, int background) {
    if (!s) return fail(MCRT_ERR_INVALID, "NULL argument");
    if (!valid_background(background)) return bad_background();
    s->background = background;
    return MCRT_OK;
}

int mcrt_scene_set_extra_lights(mcrt_scene* s, const mcrt_light_source* lights, int n) {
    if (!s) return fail(MCRT_ERR_INVALID, "NULL argument");
    if (const int rc = check_extra_lights(lights, n); rc != MCRT_OK) return rc;
    s->extra = light_set_of(lights, n);
    return MCRT_OK;
}

int mcrt_scene_extra_lights(const mcrt_scene* s, mcrt_light_source* out, int capacity) {
    if (!s) return 0;
    for (int i = 0; out && i < s->extra.n_extra && i < capacity; ++i) out[i] = s->extra.extra[i];
    return s->extra.n_extra;
}

int mcrt_owned_pixel_rows(const mcrt_config* cfg, int first, int step) {
    if (!cfg || !valid_frame(cfg)) return 0;
    Shard sh = make_shard(*cfg, first, step);
    return sh.owned_rows * cfg->tile_size;
}

}  // extern "C"
namespace {

// The extra lights of the one-shot renders the calling thread makes while a OneShotLights lives (mcrt_render_lights & co): the
// shells render_to_host creates take them.  nullptr: none.
thread_local const mcrt::LightSet* t_one_shot_lights = nullptr;
struct OneShotLights {
    explicit OneShotLights(const mcrt::LightSet* set) { t_one_shot_lights = set; }
    ~OneShotLights() { t_one_shot_lights = nullptr; }
    OneShotLights(const OneShotLights&) = delete;
    OneShotLights& operator=(const OneShotLights&) = delete;
};

struct CopySpan {  // a contiguous run: device bytes → host bytes
    const char* src;
    char* dst;
    size_t bytes;
};

int one_shot_streams(mcrt_scene* s) {
    if (!s->main_stream) HIP_TRY(hipStreamCreateWithFlags(&s->main_stream, hipStreamNonBlocking));
    if (!s->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
    return MCRT_OK;
}

size_t frame_pixels(const mcrt_config* c) { return static_cast<size_t>(c->width) * static_cast<size_t>(c->height); }

// pixel rows of tile row r of the frame
int tile_row_height(const mcrt_config& c, int r) { return std::min(c.tile_size, c.height - r * c.tile_size); }

// One rank of a host-buffer render: a scene shell on its device with the shard (rank, n_ranks) enqueued.
struct HostRank {
    mcrt_scene* scene = nullptr;
    int device = 0;
    std::vector<RowGroup> groups;
};

// Peer access between the gather root and a rank's device, both directions, once per pair and process.  false: the
// pair cannot reach each other directly (the caller falls back to per-device downloads).
bool peer_access(int root, int other) {
    if (root == other) return true;
    static std::mutex mu;
    static std::vector<std::pair<int, int>> enabled;
    std::lock_guard<std::mutex> lock(mu);
    for (const auto& pr : enabled)
        if (pr.first == root && pr.second == other) return true;
    int a = 0, b = 0;
    if (hipDeviceCanAccessPeer(&a, root, other) != hipSuccess || hipDeviceCanAccessPeer(&b, other, root) != hipSuccess || !a || !b) {
        (void)hipGetLastError();
        return false;
    }
    auto enable = [](int dev, int peer) {
        if (hipSetDevice(dev) != hipSuccess) return false;
        const hipError_t e = hipDeviceEnablePeerAccess(peer, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return false;
        (void)hipGetLastError();
        return true;
    };
    if (!enable(root, other) || !enable(other, root)) {
        (void)hipGetLastError();
        return false;
    }
    enabled.emplace_back(root, other);
    return true;
}

// Renders the frame on the given devices — rank r of N takes tile rows r, r+N, ... (cyclic: the figure sits in
// the middle rows) on devices[r] — and assembles it in `out`: float4 pixels (px_bytes = 16) or the RGBA8 plane
// quantised in the kernels' epilogue (px_bytes = 4: a quarter of the bytes on every link).
//   gather = 0: every device downloads its own rows straight into the host frame (N PCIe links in parallel,
//               no device-to-device traffic); rows that are final early travel while the rest still renders.
//   gather = 1: the ranks' packed rows go to devices[0] by peer copies (xGMI; peer access enabled once per pair — a
//               pair without it falls back to gather = 0); as each rank's rows arrive they are un-permuted into the
//               frame on the root and downloaded, so progress follows the ranks as they land.
// Progress callbacks (exactly totalTiles, done = 1..total) fire on the calling thread as rows land in `out`.
int render_to_host(const mcrt_scene_desc* desc, const mcrt_config* cfg, void* out, int px_bytes, mcrt_progress_fn progress, void* user,
                   const int* devices, int n_ranks, int gather, int background) {
    const double t0 = now_ms();
    std::vector<uint8_t> blob;
    std::string err;
    if (!flatten_scene(desc, blob, err)) return fail(MCRT_ERR_INVALID, err);
    const Shard all = make_shard(*cfg, 0, 1);
    if (n_ranks > all.tiles_y) n_ranks = all.tiles_y;  // no more ranks than tile rows
    if (n_ranks <= 1) gather = 0;
    for (int r = 1; r < n_ranks && gather; ++r)
        if (!peer_access(devices[0], devices[r])) gather = 0;
    const int W = cfg->width, T = cfg->tile_size;
    const size_t px = static_cast<size_t>(px_bytes);
    const size_t row_bytes = static_cast<size_t>(T) * W * px;
    const size_t whole_bytes = static_cast<size_t>(W) * cfg->height * px;
    const int total_tiles = all.tiles_x * all.tiles_y;
    char* out_bytes = static_cast<char*>(out);
    std::vector<HostRank> ranks(static_cast<size_t>(n_ranks));
    int rc = MCRT_OK;
    auto cleanup = [&](int code) {
        for (HostRank& r : ranks)
            if (r.scene) mcrt_scene_destroy(r.scene);  // synchronises, checks, pools the workspace
        return code;
    };
    const double t1 = now_ms();
    // ---- every rank: upload, enqueue its shard, note when which rows are final
    for (int r = 0; r < n_ranks && rc == MCRT_OK; ++r) {
        HostRank& hr = ranks[static_cast<size_t>(r)];
        hr.device = devices[r];
        rc = create_scene_from_blob(blob, hr.device, &hr.scene);
        if (rc != MCRT_OK) break;
        mcrt_scene* s = hr.scene;
        // One lane: after a render that forked internal streams the runtime serves pageable copies from its staged
        // path (1 MB chunks, ~15 GB/s: 2.3 ms per 1080p call instead of 0.8, tools/micro/hostpath.cpp), and
        // for a host-buffer render the download, not the chain of kernels, is the longer part.
        s->forced_lanes = 1;
        s->background = background;
        if (t_one_shot_lights) s->extra = *t_one_shot_lights;
        rc = one_shot_streams(s);
        if (rc != MCRT_OK) break;
        const Shard mine = make_shard(*cfg, r, n_ranks);
        const bool packed = n_ranks > 1;
        const size_t frame_bytes = packed ? static_cast<size_t>(mine.owned_rows) * row_bytes : whole_bytes;
        size_t want = frame_bytes;
        if (gather && r == 0)  // the root also holds every rank's packed rows and the assembled frame
            want = static_cast<size_t>(n_ranks) * (static_cast<size_t>((all.tiles_y + n_ranks - 1) / n_ranks) * row_bytes) + whole_bytes;
        hipError_t e = s->frame.reserve(want);
        if (e != hipSuccess) {
            rc = hip_fail(e, "frame allocation");
            break;
        }
        {   // A one-shot render plans its workspace to stay poolable: with the default budget (a third of the device) an
            // 8K / 64 spp frame would take tens of GB that no pool keeps — allocated and freed on EVERY call, and a hipMalloc
            // of that size now and then stalls for seconds (3.6-4.5 s observed, tools/gpu_hostpath_8k.py).  Below the pool's
            // limit the frame is cut into a few more passes (8K: +2 % device time) and the next call finds its buffers.
            const size_t limit = pool_limit(s->device);
            const size_t fixed = s->blob.bytes + s->frame.bytes + (static_cast<size_t>(512) << 20);  // + tile states, tables' slack
            if (limit > 2 * fixed) {
                const size_t room = (limit - fixed) / 10 * 9;
                const size_t budget = workspace_budget(s->device);
                s->budget = budget < room ? budget : room;
            }
        }
        if (r == 0) (void)hipEventRecord(s->ev[0], s->main_stream);
        rc = enqueue_render(s, cfg, r, n_ranks, packed ? MCRT_LAYOUT_PACKED : MCRT_LAYOUT_FRAME, px_bytes == 16 ? static_cast<float*>(s->frame.ptr) : nullptr,
                            px_bytes == 4 ? static_cast<uint8_t*>(s->frame.ptr) : nullptr, s->main_stream, /*may_record=*/false, &hr.groups);
        if (rc == MCRT_OK && r == 0) (void)hipEventRecord(s->ev[3], s->main_stream);
    }
    if (rc != MCRT_OK) return cleanup(rc);
    const double t2 = now_ms();
    int done_tiles = 0;
    auto report_rows = [&](const std::vector<int>& rows) {
        if (!progress) return;
        for (size_t i = 0; i < rows.size(); ++i)
            for (int x = 0; x < all.tiles_x; ++x) progress(++done_tiles, total_tiles, user);
    };
    // device bytes → host frame for a list of tile rows; `packed_rank` >= 0: the source holds only that rank's rows, packed
    auto spans_of = [&](const char* src0, const std::vector<int>& rows, int packed_rank) {
        std::vector<CopySpan> spans;
        for (size_t i = 0; i < rows.size();) {
            size_t j = i + 1;
            if (packed_rank < 0)  // consecutive tile rows of a frame-shaped source are one run
                while (j < rows.size() && rows[j] == rows[j - 1] + 1) ++j;
            size_t bytes = 0;
            for (size_t k = i; k < j; ++k) bytes += static_cast<size_t>(tile_row_height(*cfg, rows[k])) * W * px;
            const int row = rows[i];
            const size_t src_off = (packed_rank < 0 ? static_cast<size_t>(row) : static_cast<size_t>((row - packed_rank) / n_ranks)) * row_bytes;
            spans.push_back(CopySpan{src0 + src_off, out_bytes + static_cast<size_t>(row) * row_bytes, bytes});
            i = j;
        }
        return spans;
    };
    // the spans on `s`'s copy stream, straight into the caller's pages.  (Measured and rejected, profiles/r03_experiments:
    // landing the rows in a pinned ring and copying them out with several threads — 1.08 ms instead of 0.77 for resident
    // pages, 9.8 ms instead of 4.0 for pages that were never touched: eight threads faulting pages of one address space
    // serialise on its lock, while the runtime's own pinning faults them in bulk.)
    auto download = [&](mcrt_scene* s, const std::vector<CopySpan>& spans) -> hipError_t {
        hipError_t ce = hipSuccess;
        for (const CopySpan& sp : spans)
            if (ce == hipSuccess) ce = hipMemcpyAsync(sp.dst, sp.src, sp.bytes, hipMemcpyDeviceToHost, s->copy_stream);
        if (ce == hipSuccess) ce = hipStreamSynchronize(s->copy_stream);
        return ce;
    };
    hipError_t e = hipSuccess;
    if (!gather) {
        // ---- downloads: a rank's row groups in completion order.  The host waits for a group's events, then
        // copies on the (idle) copy stream; early groups travel while the GPU still renders the rest.
        auto download_group = [&](int r, size_t g) -> hipError_t {
            HostRank& hr = ranks[static_cast<size_t>(r)];
            mcrt_scene* s = hr.scene;
            hipError_t ce = hipSetDevice(hr.device);
            const RowGroup& grp = hr.groups[g];
            for (size_t i = 0; i < grp.wait.size() && ce == hipSuccess; ++i) ce = hipEventSynchronize(grp.wait[i]);
            if (ce != hipSuccess) return ce;
            return download(s, spans_of(static_cast<const char*>(s->frame.ptr), grp.rows, n_ranks == 1 ? -1 : r));
        };
        if (n_ranks == 1) {
            for (size_t g = 0; g < ranks[0].groups.size() && e == hipSuccess; ++g) {
                e = download_group(0, g);
                if (e == hipSuccess) report_rows(ranks[0].groups[g].rows);
            }
        } else {
            // one copier thread per rank (the PCIe links work in parallel); the calling thread delivers the progress calls
            std::mutex mu;
            std::condition_variable cv;
            std::vector<std::pair<int, size_t>> landed;  // (rank, group) in arrival order
            int copiers_left = n_ranks;
            hipError_t first_error = hipSuccess;
            std::vector<std::thread> copiers;
            for (int r = 0; r < n_ranks; ++r)
                copiers.emplace_back([&, r] {
                    hipError_t ce = hipSuccess;
                    for (size_t g = 0; g < ranks[static_cast<size_t>(r)].groups.size() && ce == hipSuccess; ++g) {
                        ce = download_group(r, g);
                        if (ce == hipSuccess) {
                            std::lock_guard<std::mutex> lock(mu);
                            landed.emplace_back(r, g);
                            cv.notify_one();
                        }
                    }
                    std::lock_guard<std::mutex> lock(mu);
                    if (ce != hipSuccess && first_error == hipSuccess) first_error = ce;
                    --copiers_left;
                    cv.notify_one();
                });
            size_t reported = 0;
            for (;;) {
                std::unique_lock<std::mutex> lock(mu);
                cv.wait(lock, [&] { return reported < landed.size() || copiers_left == 0; });
                if (reported < landed.size()) {
                    const std::pair<int, size_t> it = landed[reported++];
                    lock.unlock();
                    report_rows(ranks[static_cast<size_t>(it.first)].groups[it.second].rows);
                } else {
                    break;
                }
            }
            for (std::thread& t : copiers) t.join();
            e = first_error;
        }
    } else {
        // ---- peer gather to the root device; rank by rank: its packed rows arrive (xGMI), one launch un-permutes them
        // into the frame on the root, its rows travel to the host, its tiles are reported
        mcrt_scene* root = ranks[0].scene;
        const size_t rank_stride = static_cast<size_t>((all.tiles_y + n_ranks - 1) / n_ranks) * row_bytes;
        char* gathered = static_cast<char*>(root->frame.ptr);  // rank 0 rendered into slot 0 already
        char* assembled = gathered + static_cast<size_t>(n_ranks) * rank_stride;
        std::vector<hipEvent_t> unpacked(static_cast<size_t>(n_ranks), nullptr);
        for (int r = 0; r < n_ranks && e == hipSuccess; ++r) {
            HostRank& hr = ranks[static_cast<size_t>(r)];
            const Shard mine = make_shard(*cfg, r, n_ranks);
            if (r > 0) {  // behind the rank's render, on the rank's stream: its packed rows to the root's slot r
                e = hipSetDevice(hr.device);
                if (e == hipSuccess)
                    e = hipMemcpyPeerAsync(gathered + static_cast<size_t>(r) * rank_stride, ranks[0].device, hr.scene->frame.ptr, hr.device,
                                           static_cast<size_t>(mine.owned_rows) * row_bytes, hr.scene->main_stream);
                hipEvent_t sent = next_mark(hr.scene);
                if (e == hipSuccess && !sent) e = hipErrorOutOfMemory;
                if (e == hipSuccess) e = hipEventRecord(sent, hr.scene->main_stream);
                if (e == hipSuccess) e = hipSetDevice(ranks[0].device);
                if (e == hipSuccess) e = hipStreamWaitEvent(root->main_stream, sent, 0);
            }
            if (e == hipSuccess) e = hipSetDevice(ranks[0].device);
            if (e == hipSuccess)
                e = px_bytes == 16 ? launch_unpack_rows(*cfg, mine, reinterpret_cast<const float*>(gathered + static_cast<size_t>(r) * rank_stride),
                                                        reinterpret_cast<float*>(assembled), root->main_stream)
                                   : launch_unpack_rows8(*cfg, mine, reinterpret_cast<const uint8_t*>(gathered + static_cast<size_t>(r) * rank_stride),
                                                         reinterpret_cast<uint8_t*>(assembled), root->main_stream);
            unpacked[static_cast<size_t>(r)] = next_mark(root);
            if (e == hipSuccess && !unpacked[static_cast<size_t>(r)]) e = hipErrorOutOfMemory;
            if (e == hipSuccess) e = hipEventRecord(unpacked[static_cast<size_t>(r)], root->main_stream);
        }
        for (int r = 0; r < n_ranks && e == hipSuccess; ++r) {
            e = hipEventSynchronize(unpacked[static_cast<size_t>(r)]);
            std::vector<int> rows;
            for (int row = r; row < all.tiles_y; row += n_ranks) rows.push_back(row);
            if (e == hipSuccess) e = download(root, spans_of(assembled, rows, -1));
            if (e == hipSuccess) report_rows(rows);
        }
    }
    if (e != hipSuccess) return cleanup(hip_fail(e, "frame download"));
    const double t3 = now_ms();
    float kernel_ms = 0.0f;
    (void)hipSetDevice(ranks[0].device);
    (void)hipEventElapsedTime(&kernel_ms, ranks[0].scene->ev[0], ranks[0].scene->ev[3]);
    for (HostRank& hr : ranks) {
        const int c = mcrt_scene_check(hr.scene);
        if (c != MCRT_OK) rc = c;
    }
    cleanup(rc);
    if (rc != MCRT_OK) return rc;
    g_timings.flatten_ms = static_cast<float>(t1 - t0);
    g_timings.h2d_ms = static_cast<float>(t2 - t1);  // uploads, workspace checks and every launch call
    g_timings.kernel_ms = kernel_ms;                  // rank 0's pipeline on the device (hipEvents)
    g_timings.d2h_ms = static_cast<float>(t3 - t2);   // from the last launch call until the last row has landed (overlaps the render)
    g_timings.total_ms = static_cast<float>(now_ms() - t0);
    return MCRT_OK;
}

// The body of the host-buffer entry points behind their NULL-argument checks: float4 pixels (px_bytes = 16, `out` is the
// caller's out_rgba) or the RGBA8 plane (px_bytes = 4, out_rgba8).  `devices` NULL or n_devices <= 0: every visible device.
// A list's indices are checked here, before the scene is looked at; mcrt_render's single index (list_checked = false) is
// checked where the scene is uploaded, behind the scene's own checks.
int render_host_impl(const mcrt_scene_desc* desc, const mcrt_config* cfg, void* out, int px_bytes, mcrt_progress_fn progress, void* user,
                     const int* devices, int n_devices, int gather, int background, bool list_checked = true) {
    if (!valid_frame(cfg)) return MCRT_OK;  // generateTiles → empty → untouched Image (tile_renderer.cpp:144-146)
    if (!out) return fail(MCRT_ERR_INVALID, px_bytes == 16 ? "out_rgba is NULL" : "out_rgba8 is NULL");
    if (validate_config(cfg) != MCRT_OK) return MCRT_ERR_INVALID;
    const int visible = mcrt_device_count();
    if (visible <= 0) return fail(MCRT_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    std::vector<int> all;
    if (!devices || n_devices <= 0) {  // every visible device
        for (int d = 0; d < visible; ++d) all.push_back(d);
        devices = all.data();
        n_devices = visible;
    }
    for (int i = 0; i < n_devices && list_checked; ++i)
        if (devices[i] < 0 || devices[i] >= visible) return fail(MCRT_ERR_NO_DEVICE, "device index out of range");
    return render_to_host(desc, cfg, out, px_bytes, progress, user, devices, n_devices, gather ? 1 : 0, background);
}

// mcrt_render_png behind its NULL-argument checks
int render_png_impl(const mcrt_scene_desc* desc, const mcrt_config* cfg, const char* path, int device, int background) {
    if (!valid_frame(cfg)) return fail(MCRT_ERR_INVALID, "empty image");
    const size_t npix = static_cast<size_t>(cfg->width) * cfg->height;
    std::vector<uint8_t> host(npix * 4);
    // the RGBA8 plane straight from the kernels' epilogue: 4 B per pixel over PCIe (and xGMI) instead of 16
    const bool every = device == MCRT_DEVICE_ALL;
    const int rc = render_host_impl(desc, cfg, host.data(), 4, nullptr, nullptr, every ? nullptr : &device, every ? 0 : 1, 0, background);
    if (rc != MCRT_OK) return rc;
    return mcrt_write_png_rgba8(path, host.data(), cfg->width, cfg->height);
}

// One output plane of a host form: where the caller wants it (NULL: not wanted), the bytes of one element, and the pointer
// that takes its device address — a member of the struct the device form is given, of the host pointer's type (the constructor
// holds the two types together; the address goes in and out as a pointer's bytes, whatever it points to).
struct Plane {
    void* host;
    size_t elem_bytes;
    void* slot;
    template <class T>
    Plane(T* host_plane, size_t bytes, T** device_plane) : host(host_plane), elem_bytes(bytes), slot(device_plane) {}
};

// The wanted planes of `count` elements each, one after the other from `base`, every one on a 16-byte boundary (the start of
// a frame buffer is allocation-aligned).  Without a base: the bytes they take, and no slot is written.
template <size_t N>
size_t place_planes(const Plane (&planes)[N], size_t count, char* base) {
    size_t off = 0;
    for (const Plane& p : planes) {
        if (!p.host) continue;
        if (base) {
            char* at = base + off;
            std::memcpy(p.slot, &at, sizeof at);
        }
        off += (count * p.elem_bytes + 15) & ~static_cast<size_t>(15);
    }
    return off;
}

// The scene shells of a one-shot batch form, one per description, all on one device; the first one's streams and frame
// buffer serve the call.  Every shell is destroyed (synchronised, checked, a workspace pooled) when the set goes.
struct OneShotScenes {
    std::vector<mcrt_scene*> h;
    int create(const mcrt_scene_desc* const* descs, int n, int device, int background) {
        std::vector<std::vector<uint8_t>> blobs(static_cast<size_t>(n));
        for (int i = 0; i < n; ++i) {
            std::string err;
            if (!flatten_scene(descs[i], blobs[static_cast<size_t>(i)], err)) return fail(MCRT_ERR_INVALID, err);
        }
        h.assign(static_cast<size_t>(n), nullptr);
        for (int i = 0; i < n; ++i) {  // (the first one checks the device index)
            const int rc = create_scene_from_blob(blobs[static_cast<size_t>(i)], device, &h[static_cast<size_t>(i)]);
            if (rc != MCRT_OK) return rc;
            h[static_cast<size_t>(i)]->background = background;
            if (t_one_shot_lights) h[static_cast<size_t>(i)]->extra = *t_one_shot_lights;  // (the multi-light pass forms: OneShotLights)
        }
        return one_shot_streams(h[0]) == MCRT_OK ? MCRT_OK : MCRT_ERR_HIP;
    }
    // every wanted plane (count elements each, placed by place_planes) to its host address, on the first shell's stream,
    // unless the call has failed already
    template <size_t N>
    void download(const Plane (&planes)[N], size_t count, int& rc) {
        for (const Plane& p : planes) {
            if (rc != MCRT_OK || !p.host) continue;
            const void* src = nullptr;
            std::memcpy(&src, p.slot, sizeof src);
            const hipError_t e = hipMemcpyAsync(p.host, src, count * p.elem_bytes, hipMemcpyDeviceToHost, h[0]->main_stream);
            if (e != hipSuccess) rc = hip_fail(e, "download");
        }
    }
    void destroy() {
        for (mcrt_scene* s : h)
            if (s) mcrt_scene_destroy(s);
        h.clear();
    }
    OneShotScenes() = default;
    OneShotScenes(const OneShotScenes&) = delete;
    OneShotScenes& operator=(const OneShotScenes&) = delete;
    ~OneShotScenes() { destroy(); }
};

constexpr size_t kPerTexel = 0;  // one_shot_pass's count of a pass over the texels of the scene's pool (the bake), not over pixels

// A one-shot pass form behind its argument checks: the shells of the n descriptions are created, the wanted planes of `count`
// elements each (kPerTexel: the first scene's texel pool; nothing is written where that is empty) are reserved and placed in the
// first shell's frame buffer, enqueue(handles, count, stream) makes the *_batch_device call on the struct the planes' slots
// belong to, every wanted plane is downloaded and the stream synchronised.  what_planes, what_render: hip_fail's texts.
template <size_t N, class Enqueue>
int one_shot_pass(const mcrt_scene_desc* const* descs, int n, int device, const Plane (&planes)[N], size_t count, const char* what_planes,
                  const char* what_render, Enqueue enqueue) {
    OneShotScenes set;
    int rc = set.create(descs, n, device, MCRT_BACKGROUND_REFERENCE);
    if (rc != MCRT_OK) return rc;
    mcrt_scene* s0 = set.h[0];
    if (count == kPerTexel) count = static_cast<size_t>(s0->n_texels);
    if (count == 0) return MCRT_OK;
    hipError_t e = s0->frame.reserve(place_planes(planes, count, nullptr));
    if (e != hipSuccess) return hip_fail(e, what_planes);
    place_planes(planes, count, static_cast<char*>(s0->frame.ptr));
    rc = enqueue(set.h.data(), count, s0->main_stream);
    set.download(planes, count, rc);
    if (rc == MCRT_OK) {
        e = hipStreamSynchronize(s0->main_stream);
        if (e != hipSuccess) rc = hip_fail(e, what_render);
    }
    return rc;
}

}  // namespace
extern "C" {

int mcrt_render_multi(const mcrt_scene_desc* desc, const mcrt_config* cfg, float* out_rgba, mcrt_progress_fn progress, void* user,
                      const int* devices, int n_devices, int gather) {
    if (!desc || !cfg) return fail(MCRT_ERR_INVALID, "NULL argument");
    return render_host_impl(desc, cfg, out_rgba, 16, progress, user, devices, n_devices, gather, MCRT_BACKGROUND_REFERENCE);
}

int mcrt_render(const mcrt_scene_desc* desc, const mcrt_config* cfg, float* out_rgba, mcrt_progress_fn progress, void* user, int device) {
    if (device == MCRT_DEVICE_ALL) return mcrt_render_multi(desc, cfg, out_rgba, progress, user, nullptr, 0, 0);
    if (!desc || !cfg) return fail(MCRT_ERR_INVALID, "NULL argument");
    return render_host_impl(desc, cfg, out_rgba, 16, progress, user, &device, 1, 0, MCRT_BACKGROUND_REFERENCE, /*list_checked=*/false);
}

int mcrt_render_rgba8(const mcrt_scene_desc* desc, const mcrt_config* cfg, uint8_t* out_rgba8, mcrt_progress_fn progress, void* user,
                      const int* devices, int n_devices, int gather) {
    if (!desc || !cfg) return fail(MCRT_ERR_INVALID, "NULL argument");
    return render_host_impl(desc, cfg, out_rgba8, 4, progress, user, devices, n_devices, gather, MCRT_BACKGROUND_REFERENCE);
}

int mcrt_render_ex(const mcrt_scene_desc* desc, const mcrt_config* cfg, int background, float* out_rgba, uint8_t* out_rgba8,
                   mcrt_progress_fn progress, void* user, const int* devices, int n_devices, int gather) {
    if (!desc || !cfg) return fail(MCRT_ERR_INVALID, "NULL argument");
    if (!valid_background(background)) return bad_background();
    if ((out_rgba != nullptr) == (out_rgba8 != nullptr)) return fail(MCRT_ERR_INVALID, "exactly one of out_rgba / out_rgba8 must be given");
    void* out = out_rgba ? static_cast<void*>(out_rgba) : out_rgba8;
    return render_host_impl(desc, cfg, out, out_rgba ? 16 : 4, progress, user, devices, n_devices, gather, background);
}

int mcrt_render_rect(const mcrt_scene_desc* desc, const mcrt_config* cfg, const mcrt_tile* tile, float* frame_rgba, int device) {
    if (!desc || !cfg || !tile || !frame_rgba) return fail(MCRT_ERR_INVALID, "NULL argument");
    if (cfg->width <= 0 || cfg->height <= 0) return MCRT_OK;
    if (validate_config(cfg) != MCRT_OK) return MCRT_ERR_INVALID;
    if (tile->width <= 0 || tile->height <= 0) return MCRT_OK;  // renderTile's loops do not run
    if (tile->x < 0 || tile->y < 0 || tile->x > cfg->width - tile->width || tile->y > cfg->height - tile->height)
        return fail(MCRT_ERR_INVALID, "tile rectangle reaches outside the frame");
    mcrt_scene* s = nullptr;
    int rc = mcrt_scene_create(desc, device, &s);
    if (rc != MCRT_OK) return rc;
    s->forced_lanes = 1;  // one stream, like every host-buffer entry point (see render_to_host)
    const size_t row_floats = static_cast<size_t>(cfg->width) * 4;
    std::vector<float> host(row_floats * static_cast<size_t>(tile->height));
    hipError_t e = s->frame.reserve(host.size() * 4);
    if (e == hipSuccess) {
        // the rectangle is the launch's one tile; its pixel rows come back packed (full frame width)
        mcrt_config one = *cfg;
        if (one.tile_size <= 0) one.tile_size = 1;  // renderTile itself never reads tileSize
        rc = enqueue_render(s, &one, 0, 1, MCRT_LAYOUT_PACKED, static_cast<float*>(s->frame.ptr), nullptr, nullptr, /*may_record=*/false, nullptr, tile);
        if (rc == MCRT_OK) rc = mcrt_scene_check(s);
        if (rc == MCRT_OK) e = hipMemcpy(host.data(), s->frame.ptr, host.size() * 4, hipMemcpyDeviceToHost);
    }
    mcrt_scene_destroy(s);
    if (e != hipSuccess) return hip_fail(e, "render_rect");
    if (rc != MCRT_OK) return rc;
    for (int ly = 0; ly < tile->height; ++ly)
        std::memcpy(frame_rgba + 4 * (static_cast<size_t>(tile->y + ly) * cfg->width + tile->x),
                    host.data() + row_floats * static_cast<size_t>(ly) + 4 * static_cast<size_t>(tile->x), static_cast<size_t>(tile->width) * 16);
    return MCRT_OK;
}

int mcrt_render_tile(const mcrt_scene_desc* desc, const mcrt_config* cfg, int tile_index, float* frame_rgba, int device) {
    if (!desc || !cfg || !frame_rgba) return fail(MCRT_ERR_INVALID, "NULL argument");
    if (!valid_frame(cfg)) return MCRT_OK;
    Shard all = make_shard(*cfg, 0, 1);
    if (tile_index < 0 || tile_index >= all.tiles_x * all.tiles_y) return fail(MCRT_ERR_INVALID, "tile index out of range");
    const int row = tile_index / all.tiles_x, col = tile_index % all.tiles_x;
    mcrt_tile t;
    t.x = col * cfg->tile_size, t.y = row * cfg->tile_size;
    t.width = std::min(cfg->tile_size, cfg->width - t.x), t.height = std::min(cfg->tile_size, cfg->height - t.y);
    return mcrt_render_rect(desc, cfg, &t, frame_rgba, device);
}

// ---- PNG hand-off: the encoder and the file writers live in png_writer.cpp -------------------------
int mcrt_render_png(const mcrt_scene_desc* desc, const mcrt_config* cfg, const char* path, int device) {
    if (!desc || !cfg || !path) return fail(MCRT_ERR_INVALID, "NULL argument");
    return render_png_impl(desc, cfg, path, device, MCRT_BACKGROUND_REFERENCE);
}

int mcrt_render_png_ex(const mcrt_scene_desc* desc, const mcrt_config* cfg, int background, const char* path, int device) {
    if (!desc || !cfg || !path) return fail(MCRT_ERR_INVALID, "NULL argument");
    if (!valid_background(background)) return bad_background();
    return render_png_impl(desc, cfg, path, device, background);
}

// ---- extra lights, one-shot forms (mcrt.h, "extra lights") ------------------------------------------
int mcrt_render_lights(const mcrt_scene_desc* desc, const mcrt_config* cfg, const mcrt_light_source* lights, int n_lights, int background,
                       float* out_rgba, uint8_t* out_rgba8, mcrt_progress_fn progress, void* user, const int* devices, int n_devices, int gather) {
    if (!desc || !cfg) return fail(MCRT_ERR_INVALID, "NULL argument");
    if (const int rc = check_extra_lights(lights, n_lights); rc != MCRT_OK) return rc;
    const mcrt::LightSet set = light_set_of(lights, n_lights);
    const OneShotLights carried(&set);
    return mcrt_render_ex(desc, cfg, background, out_rgba, out_rgba8, progress, user, devices, n_devices, gather);
}

int mcrt_render_png_lights(const mcrt_scene_desc* desc, const mcrt_config* cfg, const mcrt_light_source* lights, int n_lights, int background,
                           const char* path, int device) {
    if (!desc || !cfg || !path) return fail(MCRT_ERR_INVALID, "NULL argument");
    if (const int rc = check_extra_lights(lights, n_lights); rc != MCRT_OK) return rc;
    const mcrt::LightSet set = light_set_of(lights, n_lights);
    const OneShotLights carried(&set);
    return mcrt_render_png_ex(desc, cfg, background, path, device);
}

int mcrt_last_timings(mcrt_timings* out) {
    if (!out) return MCRT_ERR_INVALID;
    *out = g_timings;
    return MCRT_OK;
}

// ---- batches: N frames of one config in one launch sequence (render_enqueue.cpp: render_batch_device) ----------------
int mcrt_render_batch(const mcrt_scene_desc* const* descs, int n_frames, const mcrt_config* cfg, float* out_rgba, uint8_t* out_rgba8, int device) {
    return mcrt_render_batch_ex(descs, n_frames, cfg, MCRT_BACKGROUND_REFERENCE, out_rgba, out_rgba8, device);
}

int mcrt_render_batch_ex(const mcrt_scene_desc* const* descs, int n_frames, const mcrt_config* cfg, int background, float* out_rgba,
                         uint8_t* out_rgba8, int device) {
    g_batch = BatchInfo{};
    if (n_frames < 0) return fail(MCRT_ERR_INVALID, "n_frames must be >= 0");
    if (!cfg || (n_frames > 0 && !descs)) return fail(MCRT_ERR_INVALID, "NULL argument");
    for (int i = 0; i < n_frames; ++i)
        if (!descs[i]) return fail(MCRT_ERR_INVALID, "NULL scene description in the batch");
    if (!out_rgba && !out_rgba8) return fail(MCRT_ERR_INVALID, "both outputs are NULL");
    if (!valid_background(background)) return bad_background();
    if (validate_config(cfg) != MCRT_OK) return MCRT_ERR_INVALID;
    if (n_frames == 0 || !valid_frame(cfg)) return MCRT_OK;  // zero tiles: nothing is written
    OneShotScenes set;
    int rc = set.create(descs, n_frames, device, background);
    if (rc != MCRT_OK) return rc;
    mcrt_scene* s0 = set.h[0];
    const size_t px = frame_pixels(cfg), total_px = px * static_cast<size_t>(n_frames);
    float* d_f32 = nullptr;
    uint8_t* d_u8 = nullptr;
    const Plane planes[] = {{out_rgba, 16, &d_f32}, {out_rgba8, 4, &d_u8}};
    hipError_t e = s0->frame.reserve(place_planes(planes, total_px, nullptr));
    if (e != hipSuccess) return hip_fail(e, "frame buffer");
    place_planes(planes, total_px, static_cast<char*>(s0->frame.ptr));
    rc = render_batch_device(set.h.data(), n_frames, cfg, d_f32, d_u8, px, s0->main_stream);
    const BatchInfo done = g_batch;
    set.download(planes, total_px, rc);
    if (rc == MCRT_OK) {
        e = hipStreamSynchronize(s0->main_stream);
        if (e != hipSuccess) rc = hip_fail(e, "batch render");
    }
    for (int i = 0; i < n_frames && rc == MCRT_OK; ++i) rc = mcrt_scene_check(set.h[static_cast<size_t>(i)]);
    set.destroy();
    g_batch = done;
    return rc;
}

int mcrt_last_batch_info(int* batched_frames, int* launch_sequences) {
    if (batched_frames) *batched_frames = g_batch.frames;
    if (launch_sequences) *launch_sequences = g_batch.sequences;
    return MCRT_OK;
}

int mcrt_render_layers_batch(const mcrt_scene_desc* const* descs, int n_frames, const mcrt_config* cfg, const mcrt_layers* out, int device) {
    if (n_frames < 0) return fail(MCRT_ERR_INVALID, "n_frames must be >= 0");
    if (!cfg || !out || (n_frames > 0 && !descs)) return fail(MCRT_ERR_INVALID, "NULL argument");
    for (int i = 0; i < n_frames; ++i)
        if (!descs[i]) return fail(MCRT_ERR_INVALID, "NULL scene description in the batch");
    if (no_plane(out)) return fail(MCRT_ERR_INVALID, "all four planes are NULL");
    if (n_frames == 0 || !valid_frame(cfg)) return MCRT_OK;  // zero tiles: nothing is written
    const size_t px = frame_pixels(cfg);
    mcrt_layers d{};
    const Plane planes[] = {{out->depth, 4, &d.depth}, {out->normal, 16, &d.normal}, {out->albedo, 16, &d.albedo}, {out->id, 16, &d.id}};
    return one_shot_pass(descs, n_frames, device, planes, px * static_cast<size_t>(n_frames), "layer planes", "layers render",
                         [&](mcrt_scene* const* h, size_t, hipStream_t stream) { return render_layers_batch_device(h, n_frames, cfg, &d, px, stream); });
}

int mcrt_render_layers(const mcrt_scene_desc* desc, const mcrt_config* cfg, const mcrt_layers* out, int device) {
    if (!desc) return fail(MCRT_ERR_INVALID, "NULL argument");
    const mcrt_scene_desc* one[1] = {desc};
    return mcrt_render_layers_batch(one, 1, cfg, out, device);
}

// ---- ground shadow: the one-shot host form (render_enqueue.cpp: render_ground_batch_device) and the scene's floor ------------
int mcrt_render_ground(const mcrt_scene_desc* desc, const mcrt_config* cfg, float ground_y, const mcrt_ground* out, int device) {
    if (!desc || !cfg || !out) return fail(MCRT_ERR_INVALID, "NULL argument");
    if (no_plane(out)) return fail(MCRT_ERR_INVALID, "all three planes are NULL");
    if (!std::isfinite(ground_y)) return fail(MCRT_ERR_INVALID, "ground_y must be finite");
    if (cfg->soft_shadows && cfg->shadow_samples > kGroundMaxSamples)
        return fail(MCRT_ERR_INVALID, "a ground pass takes at most 113 shadow samples (the truncated engine's 227 draws)");
    if (!valid_frame(cfg)) return MCRT_OK;  // zero tiles: nothing is written
    mcrt_ground d{};
    const Plane planes[] = {{out->visibility, 4, &d.visibility}, {out->distance, 4, &d.distance}, {out->matte, 1, &d.matte}};
    return one_shot_pass(&desc, 1, device, planes, frame_pixels(cfg), "ground planes", "ground render", [&](mcrt_scene* const* h, size_t px, hipStream_t stream) {
        return render_ground_batch_device(h, 1, cfg, &ground_y, &d, px, stream);
    });
}

// ---- ground occlusion: the one-shot host form (render_enqueue.cpp: render_ground_occlusion_batch_device) ------------------------
int mcrt_render_ground_occlusion(const mcrt_scene_desc* desc, const mcrt_config* cfg, float ground_y, const mcrt_ground_occlusion* out, int device) {
    if (!desc || !cfg || !out) return fail(MCRT_ERR_INVALID, "NULL argument");
    if (no_plane(out)) return fail(MCRT_ERR_INVALID, "both planes are NULL");
    if (!std::isfinite(ground_y)) return fail(MCRT_ERR_INVALID, "ground_y must be finite");
    if (const int rc = check_ground_occlusion_config(cfg); rc != MCRT_OK) return rc;
    if (!valid_frame(cfg)) return MCRT_OK;  // zero tiles: nothing is written
    mcrt_ground_occlusion d{};
    const Plane planes[] = {{out->occlusion, 4, &d.occlusion}, {out->matte, 1, &d.matte}};
    return one_shot_pass(&desc, 1, device, planes, frame_pixels(cfg), "ground occlusion planes", "ground occlusion render",
                         [&](mcrt_scene* const* h, size_t px, hipStream_t stream) { return render_ground_occlusion_batch_device(h, 1, cfg, &ground_y, &d, px, stream); });
}

// ---- ground reflection: the one-shot host form (render_enqueue.cpp: render_reflection_batch_device) -----------------------------
int mcrt_render_reflection(const mcrt_scene_desc* desc, const mcrt_config* cfg, float ground_y, const mcrt_reflection* out, int device) {
    if (!desc || !cfg || !out) return fail(MCRT_ERR_INVALID, "NULL argument");
    if (no_plane(out)) return fail(MCRT_ERR_INVALID, "all three planes are NULL");
    if (!std::isfinite(ground_y)) return fail(MCRT_ERR_INVALID, "ground_y must be finite");
    if (cfg->soft_shadows && cfg->shadow_samples > kGroundMaxSamples)
        return fail(MCRT_ERR_INVALID, "a reflection pass takes at most 113 shadow samples (the truncated engine's 227 draws)");
    if (cfg->max_bounces > kReflectMaxBounces) return fail(MCRT_ERR_INVALID, "a reflection pass takes at most 8 bounces (its per-lane colour stack)");
    if (!valid_frame(cfg)) return MCRT_OK;  // zero tiles: nothing is written
    mcrt_reflection d{};
    const Plane planes[] = {{out->rgba, 16, &d.rgba}, {out->distance, 4, &d.distance}, {out->rgba8, 4, &d.rgba8}};
    return one_shot_pass(&desc, 1, device, planes, frame_pixels(cfg), "reflection planes", "reflection render", [&](mcrt_scene* const* h, size_t px, hipStream_t stream) {
        return render_reflection_batch_device(h, 1, cfg, &ground_y, &d, px, stream);
    });
}

// ---- studio shot: defaults, the scratch size and the one-shot host forms (render_enqueue.cpp: render_shot_batch_device) ----------
void mcrt_shot_init(mcrt_shot* shot) {
    if (!shot) return;
    shot->page = MCRT_PAGE_REFERENCE;
    shot->page_color[0] = shot->page_color[1] = shot->page_color[2] = 1.0f;
    shot->shadow_strength = 0.6f;
    shot->reflectivity = 0.35f;
    shot->reflection_fade = 0.0f;
}

size_t mcrt_shot_scratch_bytes(const mcrt_config* cfg, const mcrt_shot* shot, int n_frames) {
    if (!cfg || !shot || n_frames <= 0 || !valid_frame(cfg) || shot_frame_too_large(cfg)) return 0;
    if (check_shot(shot) != MCRT_OK) return 0;
    return shot_scratch(cfg, shot, n_frames).bytes;
}

size_t mcrt_shot_scratch_bytes_occ(const mcrt_config* cfg, const mcrt_shot* shot, float floor_occlusion, int n_frames) {
    if (!cfg || !shot || n_frames <= 0 || !valid_frame(cfg) || shot_frame_too_large(cfg)) return 0;
    if (check_shot(shot) != MCRT_OK || check_floor_occlusion(floor_occlusion) != MCRT_OK) return 0;
    return shot_scratch(cfg, shot, n_frames, floor_occlusion).bytes;
}

void mcrt_shot_ex_init(mcrt_shot_ex* shot) {
    if (!shot) return;
    mcrt_shot_init(&shot->shot);
    shot->floor_occlusion = 0.0f;
    shot->shadow_color[0] = shot->shadow_color[1] = shot->shadow_color[2] = 0.0f;
}

size_t mcrt_shot_scratch_bytes_ex(const mcrt_config* cfg, const mcrt_shot_ex* shot, int n_frames) {
    if (!cfg || !shot || n_frames <= 0 || !valid_frame(cfg) || shot_frame_too_large(cfg)) return 0;
    if (check_shot(shot_spec_ex(shot, nullptr)) != MCRT_OK || check_floor_occlusion(shot->floor_occlusion) != MCRT_OK) return 0;
    return shot_scratch(cfg, &shot->shot, n_frames, shot->floor_occlusion).bytes;
}

// the host form of every entry family (spec.bounds: n_frames entries in HOST memory, downloaded with the image)
static int render_shot_batch_host(const mcrt_scene_desc* const* descs, int n_frames, const mcrt_config* cfg, const ShotSpec& spec, const float* ground_y,
                                  float* out_rgba, uint8_t* out_rgba8, int device) {
    const mcrt_shot* shot = spec.shot;
    const float floor_occlusion = spec.floor_occlusion;
    // the device form's checks that need no handle, before anything is created
    if (n_frames < 0) return fail(MCRT_ERR_INVALID, "n_frames must be >= 0");
    if (!cfg || !shot || (n_frames > 0 && (!descs || !ground_y))) return fail(MCRT_ERR_INVALID, "NULL argument");
    for (int i = 0; i < n_frames; ++i)
        if (!descs[i]) return fail(MCRT_ERR_INVALID, "NULL scene description in the batch");
    if (const int rc = check_shot(spec); rc != MCRT_OK) return rc;
    if (const int rc = check_floor_occlusion(floor_occlusion); rc != MCRT_OK) return rc;
    for (int i = 0; i < n_frames; ++i)
        if (!std::isfinite(ground_y[i])) return fail(MCRT_ERR_INVALID, "ground_y must be finite");
    if (!out_rgba && !out_rgba8) return fail(MCRT_ERR_INVALID, "both outputs are NULL");
    if (const int rc = check_shot_config(cfg, shot, floor_occlusion); rc != MCRT_OK) return rc;
    if (n_frames == 0 || !valid_frame(cfg)) return MCRT_OK;  // zero tiles: nothing is written
    if (shot_frame_too_large(cfg)) return fail(MCRT_ERR_INVALID, "the frame holds 2^31 pixels or more");
    OneShotScenes set;
    int rc = set.create(descs, n_frames, device, MCRT_BACKGROUND_REFERENCE);
    if (rc != MCRT_OK) return rc;
    mcrt_scene* s0 = set.h[0];
    const size_t px = frame_pixels(cfg), total_px = px * static_cast<size_t>(n_frames);
    // the scratch (a multiple of 16 bytes), then the outputs, then the bounds: n_frames elements, so a plane list of their own
    const size_t scratch_bytes = shot_scratch(cfg, shot, n_frames, floor_occlusion).bytes;
    float* d_f32 = nullptr;
    uint8_t* d_u8 = nullptr;
    ShotSpec on_device = spec;  // with the bounds in device memory
    on_device.bounds = nullptr;
    const Plane planes[] = {{out_rgba, 16, &d_f32}, {out_rgba8, 4, &d_u8}};
    const Plane boxes[] = {{spec.bounds, sizeof(int32_t[4]), &on_device.bounds}};
    const size_t out_bytes = place_planes(planes, total_px, nullptr);
    hipError_t e = s0->frame.reserve(scratch_bytes + out_bytes + place_planes(boxes, static_cast<size_t>(n_frames), nullptr));
    if (e != hipSuccess) return hip_fail(e, "shot planes");
    char* base = static_cast<char*>(s0->frame.ptr);
    place_planes(planes, total_px, base + scratch_bytes);
    place_planes(boxes, static_cast<size_t>(n_frames), base + scratch_bytes + out_bytes);
    rc = render_shot_batch_device(set.h.data(), n_frames, cfg, on_device, ground_y, base, scratch_bytes, d_f32, d_u8, px, s0->main_stream);
    set.download(planes, total_px, rc);
    set.download(boxes, static_cast<size_t>(n_frames), rc);
    if (rc == MCRT_OK) {
        e = hipStreamSynchronize(s0->main_stream);
        if (e != hipSuccess) rc = hip_fail(e, "shot render");
    }
    for (int i = 0; i < n_frames && rc == MCRT_OK; ++i) rc = mcrt_scene_check(set.h[static_cast<size_t>(i)]);
    return rc;
}

int mcrt_render_shot_batch(const mcrt_scene_desc* const* descs, int n_frames, const mcrt_config* cfg, const mcrt_shot* shot, const float* ground_y,
                           float* out_rgba, uint8_t* out_rgba8, int device) {
    return render_shot_batch_host(descs, n_frames, cfg, shot_spec(shot, 0.0f), ground_y, out_rgba, out_rgba8, device);
}

int mcrt_render_shot_batch_occ(const mcrt_scene_desc* const* descs, int n_frames, const mcrt_config* cfg, const mcrt_shot* shot, float floor_occlusion,
                               const float* ground_y, float* out_rgba, uint8_t* out_rgba8, int device) {
    return render_shot_batch_host(descs, n_frames, cfg, shot_spec(shot, floor_occlusion), ground_y, out_rgba, out_rgba8, device);
}

int mcrt_render_shot(const mcrt_scene_desc* desc, const mcrt_config* cfg, const mcrt_shot* shot, float ground_y, float* out_rgba, uint8_t* out_rgba8,
                     int device) {
    if (!desc) return fail(MCRT_ERR_INVALID, "NULL argument");
    const mcrt_scene_desc* one[1] = {desc};
    return mcrt_render_shot_batch(one, 1, cfg, shot, &ground_y, out_rgba, out_rgba8, device);
}

// spec.bounds: one entry in host memory, or nullptr
static int render_shot_png_host(const mcrt_scene_desc* desc, const mcrt_config* cfg, const ShotSpec& spec, float ground_y, const char* path, int device) {
    const mcrt_shot* shot = spec.shot;
    const float floor_occlusion = spec.floor_occlusion;
    if (!desc || !cfg || !shot || !path) return fail(MCRT_ERR_INVALID, "NULL argument");
    if (const int rc = check_shot(spec); rc != MCRT_OK) return rc;
    if (const int rc = check_floor_occlusion(floor_occlusion); rc != MCRT_OK) return rc;
    if (!std::isfinite(ground_y)) return fail(MCRT_ERR_INVALID, "ground_y must be finite");
    if (const int rc = check_shot_config(cfg, shot, floor_occlusion); rc != MCRT_OK) return rc;
    if (!valid_frame(cfg)) return fail(MCRT_ERR_INVALID, "empty image");
    if (shot_frame_too_large(cfg)) return fail(MCRT_ERR_INVALID, "the frame holds 2^31 pixels or more");
    std::vector<uint8_t> host(static_cast<size_t>(cfg->width) * static_cast<size_t>(cfg->height) * 4);
    const mcrt_scene_desc* one[1] = {desc};
    if (!spec.ex) {
        const int rc = render_shot_batch_host(one, 1, cfg, spec, &ground_y, nullptr, host.data(), device);
        if (rc != MCRT_OK) return rc;
        return mcrt_write_png_rgba8(path, host.data(), cfg->width, cfg->height);
    }
    // the cut-out's file: the box comes down with the image where the page is transparent and somebody wants it
    int32_t box[1][4] = {{0, 0, cfg->width, cfg->height}};
    ShotSpec with_box = spec;
    with_box.bounds = shot->page == MCRT_PAGE_TRANSPARENT && (spec.bounds || spec.crop) ? box : nullptr;
    const int rc = render_shot_batch_host(one, 1, cfg, with_box, &ground_y, nullptr, host.data(), device);
    if (rc != MCRT_OK) return rc;
    if (spec.bounds) std::memcpy(spec.bounds[0], box[0], sizeof box[0]);
    const int x0 = box[0][0], y0 = box[0][1], x1 = box[0][2], y1 = box[0][3];
    if (!spec.crop || x1 <= x0 || y1 <= y0) return mcrt_write_png_rgba8(path, host.data(), cfg->width, cfg->height);  // an empty box: the whole frame
    const size_t row = static_cast<size_t>(x1 - x0) * 4;
    std::vector<uint8_t> cut(row * static_cast<size_t>(y1 - y0));
    for (int y = y0; y < y1; ++y)
        std::memcpy(cut.data() + static_cast<size_t>(y - y0) * row, host.data() + (static_cast<size_t>(y) * static_cast<size_t>(cfg->width) + static_cast<size_t>(x0)) * 4, row);
    return mcrt_write_png_rgba8(path, cut.data(), x1 - x0, y1 - y0);
}

int mcrt_render_shot_batch_ex(const mcrt_scene_desc* const* descs, int n_frames, const mcrt_config* cfg, const mcrt_shot_ex* shot, const float* ground_y,
                              float* out_rgba, uint8_t* out_rgba8, int32_t (*out_bounds)[4], int device) {
    return render_shot_batch_host(descs, n_frames, cfg, shot_spec_ex(shot, out_bounds), ground_y, out_rgba, out_rgba8, device);
}

int mcrt_render_shot_png_ex(const mcrt_scene_desc* desc, const mcrt_config* cfg, const mcrt_shot_ex* shot, float ground_y, const char* path, int crop,
                            int32_t* out_bounds, int device) {
    return render_shot_png_host(desc, cfg, shot_spec_ex(shot, reinterpret_cast<int32_t(*)[4]>(out_bounds), crop != 0), ground_y, path, device);
}

int mcrt_render_shot_png(const mcrt_scene_desc* desc, const mcrt_config* cfg, const mcrt_shot* shot, float ground_y, const char* path, int device) {
    return render_shot_png_host(desc, cfg, shot_spec(shot, 0.0f), ground_y, path, device);
}

int mcrt_render_shot_png_occ(const mcrt_scene_desc* desc, const mcrt_config* cfg, const mcrt_shot* shot, float floor_occlusion, float ground_y, const char* path,
                             int device) {
    return render_shot_png_host(desc, cfg, shot_spec(shot, floor_occlusion), ground_y, path, device);
}

// ---- light layers: the one-shot host form (render_enqueue.cpp: render_light_batch_device) ----------------------------------------
int mcrt_render_light(const mcrt_scene_desc* desc, const mcrt_config* cfg, const mcrt_light_planes* out, int device) {
    if (!desc || !cfg || !out) return fail(MCRT_ERR_INVALID, "NULL argument");
    if (no_plane(out)) return fail(MCRT_ERR_INVALID, "all three planes are NULL");
    if (const int rc = check_light_config(cfg, out); rc != MCRT_OK) return rc;
    if (!valid_frame(cfg)) return MCRT_OK;  // zero tiles: nothing is written
    mcrt_light_planes d{};
    const Plane planes[] = {{out->direct, 16, &d.direct}, {out->visibility, 4, &d.visibility}, {out->occlusion, 4, &d.occlusion}};
    return one_shot_pass(&desc, 1, device, planes, frame_pixels(cfg), "light planes", "light render",
                         [&](mcrt_scene* const* h, size_t px, hipStream_t stream) { return render_light_batch_device(h, 1, cfg, &d, px, stream); });
}

// ---- light bake: the owner table (host only) and the one-shot host form (render_enqueue.cpp: bake_light_batch_device) ----------
int mcrt_bake_texel_table(const mcrt_scene_desc* desc, int32_t (*out)[4], int capacity) {
    std::vector<uint8_t> b;
    std::string err;
    if (!flatten_scene(desc, b, err)) {
        (void)fail(MCRT_ERR_INVALID, err);
        return -1;
    }
    const int n = static_cast<int>(reinterpret_cast<const FlatHeader*>(b.data())->n_texels);
    const int fill = out ? std::min(n, capacity) : 0;
    for (int i = 0; i < fill; ++i) out[i][0] = -1, out[i][1] = 0, out[i][2] = -1, out[i][3] = -1;
    std::vector<BakeFace> owners;
    bake_owner_faces(b.data(), owners);
    for (const BakeFace& f : owners)
        for (int rel = 0; rel < f.w * f.h && f.tex_off + rel < fill; ++rel) {
            int32_t* o = out[f.tex_off + rel];
            o[0] = f.code >> 3, o[1] = f.code & 7, o[2] = rel % f.w, o[3] = rel / f.w;
        }
    return n;
}

int mcrt_bake_light(const mcrt_scene_desc* desc, const mcrt_config* cfg, int grid, const mcrt_bake_planes* out, int device) {
    if (!desc || !cfg || !out) return fail(MCRT_ERR_INVALID, "NULL argument");
    if (no_plane(out)) return fail(MCRT_ERR_INVALID, "all five planes are NULL");
    if (const int rc = check_bake_config(cfg, grid, out); rc != MCRT_OK) return rc;
    mcrt_bake_planes d{};
    const Plane planes[] = {{out->position, 16, &d.position}, {out->normal, 16, &d.normal}, {out->direct, 16, &d.direct},
                            {out->visibility, 4, &d.visibility}, {out->occlusion, 4, &d.occlusion}};
    return one_shot_pass(&desc, 1, device, planes, kPerTexel, "bake planes", "light bake",
                         [&](mcrt_scene* const* h, size_t n, hipStream_t stream) { return bake_light_batch_device(h, 1, cfg, grid, &d, n, stream); });
}

// ---- light layers and bake under extra lights: the one-shot host forms (render_enqueue.cpp: render_light_multi_batch_device,
// bake_light_multi_batch_device).  The lights ride to the pooled shell like mcrt_render_lights' (OneShotLights).
int mcrt_render_light_multi(const mcrt_scene_desc* desc, const mcrt_config* cfg, const mcrt_light_source* lights, int n_lights,
                            const mcrt_light_planes_multi* out, int device) {
    if (!desc || !cfg || !out) return fail(MCRT_ERR_INVALID, "NULL argument");
    if (const int rc = check_extra_lights(lights, n_lights); rc != MCRT_OK) return rc;
    if (no_plane(out)) return fail(MCRT_ERR_INVALID, "all planes are NULL");
    {
        const mcrt_light_planes occ = occlusion_alone(out);
        if (const int rc = check_light_config(cfg, &occ); rc != MCRT_OK) return rc;
    }
    if (!valid_frame(cfg)) return MCRT_OK;  // zero tiles: nothing is written
    const mcrt::LightSet set = light_set_of(lights, n_lights);
    const OneShotLights carried(&set);
    mcrt_light_planes_multi d{};
    const Plane planes[] = {{out->direct[0], 16, &d.direct[0]}, {out->direct[1], 16, &d.direct[1]}, {out->direct[2], 16, &d.direct[2]},
                            {out->direct[3], 16, &d.direct[3]}, {out->combined, 16, &d.combined},
                            {out->visibility[0], 4, &d.visibility[0]}, {out->visibility[1], 4, &d.visibility[1]},
                            {out->visibility[2], 4, &d.visibility[2]}, {out->visibility[3], 4, &d.visibility[3]}, {out->occlusion, 4, &d.occlusion}};
    static_assert(MCRT_MAX_LIGHTS == 4, "the plane lists name every light");
    return one_shot_pass(&desc, 1, device, planes, frame_pixels(cfg), "light planes", "light render",
                         [&](mcrt_scene* const* h, size_t px, hipStream_t stream) { return render_light_multi_batch_device(h, 1, cfg, &d, px, stream); });
}

int mcrt_bake_light_multi(const mcrt_scene_desc* desc, const mcrt_config* cfg, const mcrt_light_source* lights, int n_lights, int grid,
                          const mcrt_bake_planes_multi* out, int device) {
    if (!desc || !cfg || !out) return fail(MCRT_ERR_INVALID, "NULL argument");
    if (const int rc = check_extra_lights(lights, n_lights); rc != MCRT_OK) return rc;
    if (no_plane(out)) return fail(MCRT_ERR_INVALID, "all planes are NULL");
    {
        const mcrt_bake_planes occ = occlusion_alone(out);
        if (const int rc = check_bake_config(cfg, grid, &occ); rc != MCRT_OK) return rc;
    }
    const mcrt::LightSet set = light_set_of(lights, n_lights);
    const OneShotLights carried(&set);
    mcrt_bake_planes_multi d{};
    const Plane planes[] = {{out->position, 16, &d.position}, {out->normal, 16, &d.normal},
                            {out->direct[0], 16, &d.direct[0]}, {out->direct[1], 16, &d.direct[1]}, {out->direct[2], 16, &d.direct[2]},
                            {out->direct[3], 16, &d.direct[3]}, {out->combined, 16, &d.combined},
                            {out->visibility[0], 4, &d.visibility[0]}, {out->visibility[1], 4, &d.visibility[1]},
                            {out->visibility[2], 4, &d.visibility[2]}, {out->visibility[3], 4, &d.visibility[3]}, {out->occlusion, 4, &d.occlusion}};
    return one_shot_pass(&desc, 1, device, planes, kPerTexel, "bake planes", "light bake",
                         [&](mcrt_scene* const* h, size_t n, hipStream_t stream) { return bake_light_multi_batch_device(h, 1, cfg, grid, &d, n, stream); });
}

int mcrt_scene_floor(const mcrt_scene_desc* desc, float* y) {
    if (!desc || !y) return fail(MCRT_ERR_INVALID, "NULL argument");
    bool any = false;
    float lowest = 0.0f;
    for (int32_t m = 0; m < desc->n_meshes && desc->meshes; ++m) {
        const mcrt_mesh& mesh = desc->meshes[m];
        if (!mesh.tri_vertices) continue;
        for (int64_t v = 0; v < static_cast<int64_t>(mesh.n_triangles) * 3; ++v) {
            const float vy = mesh.tri_vertices[3 * v + 1];
            if (!any || vy < lowest) lowest = vy;
            any = true;
        }
    }
    if (!any) return fail(MCRT_ERR_INVALID, "the scene holds no vertex");
    *y = lowest;
    return MCRT_OK;
}

int mcrt_scene_pick(mcrt_scene* s, const mcrt_config* cfg, const int32_t* xy, int n, mcrt_surface* out) {
    if (!s || !cfg) return fail(MCRT_ERR_INVALID, "NULL argument");
    if (n < 0) return fail(MCRT_ERR_INVALID, "n must be >= 0");
    if (n == 0) return MCRT_OK;
    if (!xy || !out) return fail(MCRT_ERR_INVALID, "NULL argument");
    for (int i = 0; i < n; ++i)
        if (!valid_frame(cfg) || xy[2 * i] < 0 || xy[2 * i] >= cfg->width || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= cfg->height)
            return fail(MCRT_ERR_INVALID, "a pick coordinate lies outside the frame");
    LayersShape shape;
    if (!make_layers_shape(*cfg, shape)) return fail(MCRT_ERR_INVALID, "the frame holds more than 2^31 work units");
    HIP_TRY(hipSetDevice(s->device));
    const size_t xy_bytes = (static_cast<size_t>(n) * 8 + 63) & ~static_cast<size_t>(63);
    HIP_TRY(s->pick.reserve(xy_bytes + static_cast<size_t>(n) * sizeof(mcrt_surface)));
    int32_t* d_xy = static_cast<int32_t*>(s->pick.ptr);
    mcrt_surface* d_out = reinterpret_cast<mcrt_surface*>(static_cast<char*>(s->pick.ptr) + xy_bytes);
    HIP_TRY(hipMemcpy(d_xy, xy, static_cast<size_t>(n) * 8, hipMemcpyHostToDevice));
    hipError_t e = launch_pick(static_cast<const uint8_t*>(s->blob.ptr), shape, d_xy, n, d_out, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, d_out, static_cast<size_t>(n) * sizeof(mcrt_surface), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "pick");
    return MCRT_OK;
}

}  // extern "C"
