// device_stores.cpp — what libmcrt.so keeps per device or per process: the devices' memory sizes, the live list of scene
// shells, the seed tables, the background and draw plates, the pool of idle shells and the ring of parameter tables.  Each store
// has a mutex of its own, and no function here holds one while it takes another.
#include "host_internal.h"

#include <algorithm>
#include <climits>
#include <cstring>
#include <mutex>

using namespace mcrt;

namespace mcrt_host {

// total memory of a device, asked once per device and process (hipMemGetInfo costs ~10 ms per call on this runtime: asked per
// scene it made every one-shot render 12 ms longer)
size_t device_total_memory(int device) {
    static std::mutex mu;
    static std::vector<size_t> totals;
    std::lock_guard<std::mutex> lock(mu);
    if (device < 0) return 0;
    if (totals.size() <= static_cast<size_t>(device)) totals.resize(static_cast<size_t>(device) + 1, 0);
    size_t& t = totals[static_cast<size_t>(device)];
    if (t == 0) {
        size_t total_b = 0;
        if (hipDeviceTotalMem(&total_b, device) != hipSuccess) {
            (void)hipGetLastError();
            total_b = static_cast<size_t>(24) << 30;
        }
        t = total_b ? total_b : 1;
    }
    return t;
}

// Every shell of the process (pooled ones included).  A render sizes its launches by whether its device is busy with
// another handle's frame at the moment it is enqueued (choose_grids): it asks the other shells' last-render events.
namespace {
std::mutex g_live_mutex;
std::vector<mcrt_scene*> g_live;
void unregister_live(mcrt_scene* s) {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    g_live.erase(std::remove(g_live.begin(), g_live.end(), s), g_live.end());
}
}  // namespace
void register_live(mcrt_scene* s) {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    g_live.push_back(s);
}
bool device_shared(const mcrt_scene* s) {
    static const int forced = [] {  // development knob: MCRT_SHARED_GRIDS=0 / 1 fixes the answer
        const int v = env_int("MCRT_SHARED_GRIDS", INT_MIN);
        return v == INT_MIN ? -1 : (v != 0 ? 1 : 0);
    }();
    if (forced >= 0) return forced != 0;
    bool shared = false;
    {
        std::lock_guard<std::mutex> lock(g_live_mutex);
        for (const mcrt_scene* q : g_live) {
            if (q == s || q->device != s->device) continue;
            hipEvent_t e = q->busy_probe.load(std::memory_order_acquire);
            if (e && hipEventQuery(e) == hipErrorNotReady) {
                shared = true;
                break;
            }
        }
    }
    (void)hipGetLastError();  // hipErrorNotReady is an answer, not a failure of this render
    return shared;
}

// ---- per-device seed tables (kernels.h): mt[397] of mt19937's seeding recurrence by seed, so that the kernels look up what
// they would otherwise run 397 steps for.  Two tables of one shape — by device, built on first use (synchronously, on the
// null stream), a `users` count of the scene shells, live or pooled, that hold the pointer, freed by mcrt_trim() when
// nobody does — that differ in what is below.  No table (the knob, no room, a failed build): the kernels seed by the recurrence.
// The sample table (kernels.h: a hit's light-disk samples by shadow seed) is a third of the same shape, but `sighted`: built by
// the plates' rule, at the device's second asking render (the knob at 2: the first) — a one-shot call never allocates — on a
// non-blocking stream of its own that is waited for before the asking render enqueues anything, never on the null stream.
namespace {
struct SeedTables {
    const char* knob;                 // environment variable: 0 turns the table off
    size_t bytes;
    bool small_part_only;             // built only where it is a small part of what is free (a third at most)
    hipError_t (*fill)(uint32_t* p, hipStream_t stream);  // the launches that fill it
    bool sighted;                     // the plates' rule (above)
    struct Table {
        uint32_t* ptr = nullptr;
        int users = 0;
        int sightings = 0;            // (sighted) asking renders so far; negative after a failed build: that many are waited out
        int builds = 0;               // times the table has been built (mcrt_sample_table_info)
    };
    std::vector<Table> by_device;     // (g_seed_mutex)
    int mode = -1;                    // the knob, read at the first acquire: 0 off, 2 (sighted) build at the first asking, else 1

    const uint32_t* acquire(int device, bool count_sighting = true);
    const uint32_t* acquire_built(int device);  // only where the table exists: builds nothing
    void release(int device);
    void free_unused();
};
std::mutex g_seed_mutex;
constexpr int kTableRetryAfter = 16;  // asking renders a sighted table waits after a failed build (no room, for one) before the next try

const uint32_t* SeedTables::acquire(int device, bool count_sighting) {
    std::lock_guard<std::mutex> lock(g_seed_mutex);
    if (mode < 0) {
        const int v = env_int(knob, 1);
        mode = v == 0 ? 0 : (v == 2 ? 2 : 1);
    }
    if (!mode) return nullptr;
    if (by_device.size() <= static_cast<size_t>(device)) by_device.resize(static_cast<size_t>(device) + 1);
    Table& t = by_device[static_cast<size_t>(device)];
    if (!t.ptr) {
        if (sighted) {
            if (count_sighting) ++t.sightings;
            if (t.sightings < (mode == 2 ? 1 : 2)) return nullptr;
        }
        size_t free_b = 0, total_b = 0;
        uint32_t* p = nullptr;
        hipStream_t stream = nullptr;  // (sighted: a stream of the build's own)
        const bool room = !small_part_only || (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b >= bytes * 3);
        const bool built = room && (!sighted || hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess) && hipMalloc(&p, bytes) == hipSuccess &&
                           fill(p, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
        if (stream) (void)hipStreamDestroy(stream);
        if (!built) {
            (void)hipGetLastError();
            if (p) (void)hipFree(p);
            if (sighted) t.sightings = -kTableRetryAfter;
            return nullptr;
        }
        t.ptr = p;
        ++t.builds;
    }
    ++t.users;
    return t.ptr;
}
const uint32_t* SeedTables::acquire_built(int device) {
    std::lock_guard<std::mutex> lock(g_seed_mutex);
    if (device < 0 || static_cast<size_t>(device) >= by_device.size()) return nullptr;
    Table& t = by_device[static_cast<size_t>(device)];
    if (!t.ptr) return nullptr;
    ++t.users;
    return t.ptr;
}
void SeedTables::release(int device) {
    std::lock_guard<std::mutex> lock(g_seed_mutex);
    if (static_cast<size_t>(device) < by_device.size() && by_device[static_cast<size_t>(device)].users > 0) --by_device[static_cast<size_t>(device)].users;
}
void SeedTables::free_unused() {  // mcrt_trim
    std::lock_guard<std::mutex> lock(g_seed_mutex);
    for (size_t d = 0; d < by_device.size(); ++d) {
        Table& t = by_device[d];
        if (t.ptr && t.users == 0) {
            (void)hipSetDevice(static_cast<int>(d));
            (void)hipFree(t.ptr);
            t.ptr = nullptr;
            t.sightings = 0;
        }
    }
}

// The window table: kSeedWindow words, the seeds of a frame's tiles and hits; one ~2 ms kernel.  MCRT_SEED_TABLE=0 turns it off.
SeedTables g_window_tables{"MCRT_SEED_TABLE", static_cast<size_t>(kSeedWindow) * 4, false, [](uint32_t* p, hipStream_t st) { return launch_build_seed_table(p, st); }, false};
// The table for EVERY seed: mt[397] of all 2^32 seeds, 16 GiB of the device's HBM.  The ambient-occlusion seeds,
// (unsigned)(P.x * 73856093 + P.y * 19349663 + P.z * 83492791) (raytracer.cpp:122-123), cover the whole 32-bit range, and the
// 397-step recurrence is over a quarter of the AO stage's cycles (its multiply issues at a quarter of the rate).  Built on
// a device's first AO render (0.2 s), when the device has the room; MCRT_AO_SEED_TABLE=0 turns it off.
SeedTables g_full_tables{"MCRT_AO_SEED_TABLE", static_cast<size_t>(1) << 34, true, [](uint32_t* p, hipStream_t st) {
                             hipError_t e = hipSuccess;
                             for (uint32_t part = 0; part < 16u && e == hipSuccess; ++part) e = launch_build_seed_table_range(p, part << 28, 1u << 28, st);
                             return e;
                         }, false};
// The sample table: kSampleWindow rows of 128 bytes, 1 GiB, the light-disk samples of the seeds a character scene's hits have;
// one kernel of about a millisecond.  MCRT_SAMPLE_TABLE=0 turns it off, =2 builds it at the device's first asking render.
SeedTables g_sample_tables{"MCRT_SAMPLE_TABLE", static_cast<size_t>(kSampleWindow) * kSampleRow * sizeof(float4), true,
                           [](uint32_t* p, hipStream_t st) { return launch_build_sample_table(reinterpret_cast<float4*>(p), st); }, true};
}  // namespace

const uint32_t* acquire_seed_table(int device) { return g_window_tables.acquire(device); }
void ensure_full_seed_table(mcrt_scene* s, hipStream_t stream) {
    if (s->full_table_tried) return;
    if (stream_capturing(stream)) return;  // (building it launches and waits)
    s->full_table_tried = true;
    s->seed_table_full = g_full_tables.acquire(s->device);
    s->holds_full_table = s->seed_table_full != nullptr;
}
// The shell takes the device's sample table at a render whose soft shadows a row can serve (2 .. kSampleRow samples), building
// it by the sighting rule; a render the caller is capturing takes none and builds none.
static const float4* sample_table_for(mcrt_scene* s, const RenderParams& p, bool capturing, bool count_sighting) {
    if (capturing) return nullptr;
    if (!s->holds_sample_table && p.cfg.soft_shadows && p.cfg.shadow_samples > 1 && p.cfg.shadow_samples <= kSampleRow) {
        s->sample_table = reinterpret_cast<const float4*>(g_sample_tables.acquire(s->device, count_sighting));
        s->holds_sample_table = s->sample_table != nullptr;
    }
    return s->sample_table;
}
bool copy_sample_rows(int device, const int32_t* seeds, int n, float* out) {
    const uint32_t* table = g_sample_tables.acquire(device);
    if (!table) table = g_sample_tables.acquire(device);  // (the second asking builds)
    if (!table) return false;
    bool ok = true;
    constexpr size_t row_bytes = kSampleRow * sizeof(float4);
    for (int i = 0; i < n && ok; ++i) {
        const uint32_t row = static_cast<uint32_t>(seeds[i]) + kSampleWindowHalf;
        ok = row < kSampleWindow && hipMemcpy(reinterpret_cast<char*>(out) + static_cast<size_t>(i) * row_bytes,
                                              reinterpret_cast<const char*>(table) + static_cast<size_t>(row) * row_bytes, row_bytes, hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (!ok) (void)hipGetLastError();
    g_sample_tables.release(device);
    return ok;
}
bool copy_seed_words(int device, int which, const uint32_t* seeds, int n, uint32_t* out) {
    SeedTables& store = which == MCRT_TABLE_FULL ? g_full_tables : g_window_tables;
    const uint32_t* table = store.acquire(device);
    if (!table) return false;
    const uint32_t bias = which == MCRT_TABLE_FULL ? 0u : kSeedWindowHalf;  // the window table: seed s at index s + kSeedWindowHalf
    bool ok = true;
    for (int i = 0; i < n && ok; ++i) {
        const uint32_t slot = seeds[i] + bias;
        ok = (which == MCRT_TABLE_FULL || slot < kSeedWindow) && hipMemcpy(out + i, table + slot, 4, hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (!ok) (void)hipGetLastError();
    store.release(device);
    return ok;
}
void share_full_seed_table(mcrt_scene* s) {
    if (s->holds_full_table) return;
    s->seed_table_full = g_full_tables.acquire_built(s->device);
    s->holds_full_table = s->seed_table_full != nullptr;
    if (s->holds_full_table) s->full_table_tried = true;
}

namespace {
// ---- per-device plates (kernels.h; mcrt.h states the memory cost and the knobs) -------------------------------------
// Two kinds — the background tiles' pixels, every tile's draws — in one store: per kind and device a list of entries with a
// `users` count like the seed tables, all under one mutex; the kinds differ in the table below (key, bytes, fill launch,
// budget, knob).  An entry starts as a sighting record (no memory); the plate is built at the key's second render call on
// the device — one-shot calls and sweeps over thousands of sizes never allocate — synchronously, on the store's own
// non-blocking stream, never on the null stream and never while the caller records a graph.  Once built a plate is
// immutable: no validity flags, nothing published or tested on the device, no writer beside a reader.  Plates nobody holds
// make way, least recently used first, when a new one needs the room; one that does not fit gets no plate and the frame
// renders as it always did.
constexpr int kPlateKeys = 32;        // entries per kind and device, sighting records included
constexpr int kPlateRetryAfter = 16;  // sightings a key waits after a failed build before the next try
constexpr size_t kHeldPlates = 4;     // plates of a kind one scene shell holds at a time (as many as it records launch graphs)

PlateKey pixel_key_of(const RenderParams& p) {
    PlateKey k;
    std::memset(&k, 0, sizeof k);
    k.width = p.cfg.width, k.height = p.cfg.height, k.tile_size = p.cfg.tile_size;
    k.spp = p.cfg.samples_per_pixel > 1 ? p.cfg.samples_per_pixel : 1;
    k.draws_per_sample = p.draws_per_sample;
    k.gradient_bg = p.cfg.gradient_bg ? 1 : 0;
    k.div_frame = p.div_frame;
    k.gradient_scale = p.cfg.gradient_scale;
    for (int i = 0; i < 3; ++i) k.bg_center[i] = p.cfg.bg_center[i], k.bg_edge[i] = p.cfg.bg_edge[i];
    return k;
}
PlateKey draw_key_of(const RenderParams& p) {  // a tile's draws: the frame's size, the tile size, the samples and the draws per sample
    PlateKey k;
    std::memset(&k, 0, sizeof k);
    k.width = p.cfg.width, k.height = p.cfg.height, k.tile_size = p.cfg.tile_size;
    k.spp = p.cfg.samples_per_pixel > 1 ? p.cfg.samples_per_pixel : 1;
    k.draws_per_sample = p.draws_per_sample;
    return k;
}
bool same_key(const PlateKey& a, const PlateKey& b) { return std::memcmp(&a, &b, sizeof a) == 0; }  // (floats by their bits)

struct PlateKindInfo {
    const char* knob;   // development knob: 0 no plates, 2 build at a key's first render (tests); else at the second
    size_t budget;      // built plates of a device, together
    int max_built;      // built plates per device
    bool (*eligible)(const RenderParams& p);
    PlateKey (*key_of)(const RenderParams& p);
    size_t (*bytes)(const RenderParams& p);
    size_t (*rng_bytes)(const RenderParams& p);  // scratch of the fill: the engine states of every tile of the frame
    hipError_t (*fill)(const RenderParams& p, void* plate, uint32_t* rng, hipStream_t stream);
    int mode = -1;      // the knob, read once (plate_mode)
};
PlateKindInfo g_kinds[kPlateKinds] = {
    {"MCRT_BG_PLATE", static_cast<size_t>(MCRT_BG_PLATE_BUDGET_MB) << 20, 8, bg_plate_eligible, pixel_key_of,
     [](const RenderParams& p) { return bg_plate_bytes(p.cfg); }, bg_plate_rng_bytes,
     [](const RenderParams& p, void* plate, uint32_t* rng, hipStream_t st) { return launch_fill_bg_plate(p, static_cast<float4*>(plate), rng, st); }},
    {"MCRT_DRAW_PLATE", static_cast<size_t>(MCRT_DRAW_PLATE_BUDGET_MB) << 20, 4, draw_plate_eligible, draw_key_of, draw_plate_bytes, draw_plate_rng_bytes,
     [](const RenderParams& p, void* plate, uint32_t* rng, hipStream_t st) { return launch_fill_draw_plate(p, static_cast<float*>(plate), rng, st); }},
};
struct DevicePlates {
    std::vector<Plate*> entries;
    unsigned long long clock = 0;
    hipStream_t stream = nullptr;  // the builds
    size_t bytes = 0;              // of the built plates
    int built = 0;
    int builds = 0;                // plates built so far (mcrt_bg_plate_info, mcrt_draw_plate_info)
};
std::mutex g_plate_mutex;
std::vector<DevicePlates> g_plates[kPlateKinds];  // by device

int plate_mode(int kind) {
    static std::once_flag once;
    std::call_once(once, [] {
        for (PlateKindInfo& k : g_kinds) {
            const int v = env_int(k.knob, 1);
            k.mode = v == 0 ? 0 : (v == 2 ? 2 : 1);
        }
    });
    return g_kinds[kind].mode;
}

// g_plate_mutex held.  Frees a built plate nobody holds: every holder synchronised the device before it let go.
void free_plate(DevicePlates& d, Plate* e) {
    if (!e->ptr) return;
    (void)hipFree(e->ptr);
    e->ptr = nullptr;
    d.bytes -= e->bytes;
    e->bytes = 0;
    --d.built;
}
// g_plate_mutex held, the device current.  Builds e's plate for the frame prepared as `p`; leaves e->ptr NULL when there is no room
// (false is returned; asked again at the key's next render) or the build fails (an allocation refused, for one: asked again
// kPlateRetryAfter sightings later).
bool build_plate(const PlateKindInfo& kind, DevicePlates& d, Plate* e, const RenderParams& p, size_t bytes) {
    while (d.built >= kind.max_built || d.bytes + bytes > kind.budget) {
        Plate* victim = nullptr;
        for (Plate* q : d.entries)
            if (q != e && q->ptr && q->users == 0 && (!victim || q->last_use < victim->last_use)) victim = q;
        if (!victim) return false;
        free_plate(d, victim);
        victim->sightings = 0;
    }
    void* plate = nullptr;
    uint32_t* rng = nullptr;
    hipError_t err = d.stream ? hipSuccess : hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking);
    if (err == hipSuccess) err = hipMalloc(&plate, bytes);
    if (err == hipSuccess) err = hipMalloc(&rng, kind.rng_bytes(p));
    if (err == hipSuccess) err = kind.fill(p, plate, rng, d.stream);
    if (err == hipSuccess) err = hipStreamSynchronize(d.stream);
    if (rng) (void)hipFree(rng);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        if (plate) (void)hipFree(plate);
        e->sightings = -kPlateRetryAfter;
        return true;
    }
    e->ptr = plate;
    e->bytes = bytes;
    d.bytes += bytes;
    ++d.built;
    ++d.builds;
    return true;
}
// The shell lets go of the plate of `kind` it has held longest.  Its launches in flight and its recorded launch graphs may
// read the plate: its last render is waited for — every render of a handle ends in `last_done`, lanes joined, and a
// handle's renders run one after the other, so nothing of this handle reads the plate after it; other handles' frames are
// not waited for — and those graphs are dropped first.
void drop_held_plate(mcrt_scene* s, int kind) {
    Plate* e = s->plates[kind].front();
    if (s->have_last && s->last_done) (void)hipEventSynchronize(s->last_done);
    for (auto& r : s->recorded) {
        bool reads = false;
        for (int li = 0; li < kMaxLanes; ++li) {
            const void* read = kind == kPlatePixels ? static_cast<const void*>(r.p[li].bg_plate) : static_cast<const void*>(r.p[li].draw_plate);
            reads = reads || (read != nullptr && read == e->ptr);
        }
        if (!reads) continue;
        if (r.exec) (void)hipGraphExecDestroy(r.exec);
        if (r.graph) (void)hipGraphDestroy(r.graph);
        r.exec = nullptr;
        r.graph = nullptr;
        r.n_lanes = 0;
        r.sightings = 0;
    }
    s->plates[kind].erase(s->plates[kind].begin());
    std::lock_guard<std::mutex> lock(g_plate_mutex);
    --e->users;
}
void release_plates(mcrt_scene* s) {  // the shell goes (its device work has been waited for)
    std::lock_guard<std::mutex> lock(g_plate_mutex);
    for (auto& held : s->plates) {
        for (Plate* e : held) --e->users;
        held.clear();
    }
}

void free_unused_plates() {  // mcrt_trim
    std::lock_guard<std::mutex> lock(g_plate_mutex);
    for (auto& by_device : g_plates)
        for (size_t dev = 0; dev < by_device.size(); ++dev) {
            DevicePlates& d = by_device[dev];
            (void)hipSetDevice(static_cast<int>(dev));
            std::vector<Plate*> kept;
            for (Plate* e : d.entries) {
                if (e->users > 0) {
                    kept.push_back(e);
                    continue;
                }
                free_plate(d, e);
                delete e;
            }
            d.entries.swap(kept);
            if (d.stream) (void)hipStreamDestroy(d.stream);  // idle: every build waited for it under this mutex
            d.stream = nullptr;
        }
}

// the device's plate of `kind` for the frame prepared as `p`, or nullptr
const void* acquire_plate(int kind, mcrt_scene* s, const RenderParams& p, bool capturing, bool count_sighting) {
    const int mode = plate_mode(kind);
    const PlateKindInfo& info = g_kinds[kind];
    // (a caller's graph outlives this call in ways the library cannot see: a render recorded into it takes no plate)
    if (mode == 0 || capturing || !info.eligible(p)) return nullptr;
    const PlateKey key = info.key_of(p);
    std::vector<Plate*>& held = s->plates[kind];
    for (size_t i = 0; i < held.size(); ++i)
        if (same_key(held[i]->key, key)) {  // held already: no lock, the entry cannot change under a holder
            Plate* e = held[i];
            held.erase(held.begin() + static_cast<long>(i));
            held.push_back(e);
            return e->ptr;
        }
    const size_t bytes = info.bytes(p);
    if (bytes == 0 || bytes > info.budget) return nullptr;
    Plate* got = nullptr;
    // A shell may hold as many plates as the device keeps of a kind: when the store has no room because every built plate is
    // held, the shell lets go of the one it has held longest and asks once more (a handle that goes through many
    // configurations moves on with them instead of keeping the plates of its first ones for good).
    for (int attempt = 0; attempt < 2 && !got; ++attempt) {
        if (attempt == 1) {
            if (held.empty()) break;
            drop_held_plate(s, kind);
        }
        bool room = true;
        std::lock_guard<std::mutex> lock(g_plate_mutex);
        std::vector<DevicePlates>& by_device = g_plates[kind];
        if (by_device.size() <= static_cast<size_t>(s->device)) by_device.resize(static_cast<size_t>(s->device) + 1);
        DevicePlates& d = by_device[static_cast<size_t>(s->device)];
        ++d.clock;
        Plate* e = nullptr;
        for (Plate* q : d.entries)
            if (same_key(q->key, key)) e = q;
        if (!e) {
            if (d.entries.size() >= static_cast<size_t>(kPlateKeys)) {  // the least recently used entry nobody holds becomes this key's
                for (Plate* q : d.entries)
                    if (q->users == 0 && (!e || q->last_use < e->last_use)) e = q;
                if (!e) return nullptr;
                free_plate(d, e);
                *e = Plate{};
            } else {
                e = new Plate();
                d.entries.push_back(e);
            }
            e->key = key;
        }
        e->last_use = d.clock;
        if (!e->ptr) {
            if (count_sighting && attempt == 0) ++e->sightings;
            if (e->sightings >= (mode == 2 ? 1 : 2)) room = build_plate(info, d, e, p, bytes);
        }
        if (e->ptr) {
            ++e->users;
            got = e;
        }
        if (room) break;
    }
    if (!got) return nullptr;
    if (held.size() >= kHeldPlates) drop_held_plate(s, kind);
    held.push_back(got);
    return got->ptr;
}

int plate_info(int kind, int device, int* plates, size_t* bytes, int* builds) {
    std::lock_guard<std::mutex> lock(g_plate_mutex);
    const std::vector<DevicePlates>& by_device = g_plates[kind];
    const DevicePlates* d = (device >= 0 && static_cast<size_t>(device) < by_device.size()) ? &by_device[static_cast<size_t>(device)] : nullptr;
    if (plates) *plates = d ? d->built : 0;
    if (bytes) *bytes = d ? d->bytes : 0;
    if (builds) *builds = d ? d->builds : 0;
    return MCRT_OK;
}
}  // namespace

void acquire_plates(mcrt_scene* s, RenderParams* p, int n, bool capturing, bool count_sighting) {
    const float4* pixels = static_cast<const float4*>(acquire_plate(kPlatePixels, s, p[0], capturing, count_sighting));
    const float* draws = static_cast<const float*>(acquire_plate(kPlateDraws, s, p[0], capturing, count_sighting));
    const float4* samples = sample_table_for(s, p[0], capturing, count_sighting);
    for (int i = 0; i < n; ++i) p[i].bg_plate = pixels, p[i].draw_plate = draws, p[i].sample_table = samples;
}

// ---- per-device repaint tables (kernels.h: SkinPaintShape), one per skin kind: the 256 floats i / 255.0f — formed HERE, on
// the host, by the scene builder's own expression, so a repainted texel is the builder's float whatever the device's divide
// does — then per pool texel (mesh << 12) | skin pixel, from the builder's tables (scene_builder.cpp).  6.6, 4.9 and 6.3 KB;
// a `users` count of the handles that hold them, like the seed tables.
extern "C" int mcrt_detail_skin_pool(int skin_height, int model, int32_t* pixel, int32_t* mesh_of, int capacity);  // scene_builder.cpp
namespace {
struct SkinTables {
    void* ptr = nullptr;
    int users = 0;
};
std::mutex g_skin_mutex;
std::vector<SkinTables> g_skin_tables[kSkinKinds];  // [skin_kind_index], by device
}  // namespace

const void* acquire_skin_tables(int device, int skin_height, int model) {
    std::lock_guard<std::mutex> lock(g_skin_mutex);
    std::vector<SkinTables>& by_device = g_skin_tables[skin_kind_index(skin_height, model)];
    if (by_device.size() <= static_cast<size_t>(device)) by_device.resize(static_cast<size_t>(device) + 1);
    SkinTables& t = by_device[static_cast<size_t>(device)];
    if (!t.ptr) {
        int32_t pixel[kSkinMaxTexels], mesh_of[kSkinMaxTexels];
        const int n = mcrt_detail_skin_pool(skin_height, model, pixel, mesh_of, kSkinMaxTexels);  // (writes kSkinMaxTexels entries at most)
        if (n <= 0 || n > kSkinMaxTexels) return nullptr;  // the builder's tables outgrew the kernel's: no repaint, never an over-read
        std::vector<uint8_t> host(skin_tables_bytes(n));
        float* unit = reinterpret_cast<float*>(host.data());
        for (int i = 0; i < 256; ++i) unit[i] = static_cast<uint8_t>(i) / 255.0f;  // image.cpp:16-21, as mcrt_build_skin_scene
        uint16_t* map = reinterpret_cast<uint16_t*>(unit + 256);
        for (int i = 0; i < n; ++i) map[i] = static_cast<uint16_t>((mesh_of[i] << 12) | pixel[i]);
        void* p = nullptr;
        if (hipMalloc(&p, host.size()) != hipSuccess || hipMemcpy(p, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            if (p) (void)hipFree(p);
            return nullptr;
        }
        t.ptr = p;
    }
    ++t.users;
    return t.ptr;
}
void release_skin_tables(int device, int skin_height, int model) {
    std::lock_guard<std::mutex> lock(g_skin_mutex);
    std::vector<SkinTables>& by_device = g_skin_tables[skin_kind_index(skin_height, model)];
    if (static_cast<size_t>(device) < by_device.size() && by_device[static_cast<size_t>(device)].users > 0) --by_device[static_cast<size_t>(device)].users;
}
// ---- and the cape's (kernels.h: CapePaintShape), one per device: the same 256 floats, then per texel of the cape mesh its
// cape pixel, from the builder's map (scene_builder.cpp).  2.5 KB.
extern "C" int mcrt_cape_pool_map(int32_t* out, int capacity);  // scene_builder.cpp
namespace {
std::vector<SkinTables> g_cape_tables;  // by device (g_skin_mutex)
}
const void* acquire_cape_tables(int device) {
    std::lock_guard<std::mutex> lock(g_skin_mutex);
    if (g_cape_tables.size() <= static_cast<size_t>(device)) g_cape_tables.resize(static_cast<size_t>(device) + 1);
    SkinTables& t = g_cape_tables[static_cast<size_t>(device)];
    if (!t.ptr) {
        int32_t pixel[kCapeTexels];
        if (mcrt_cape_pool_map(pixel, kCapeTexels) != kCapeTexels) return nullptr;  // the builder's map outgrew the kernel's: no repaint
        std::vector<uint8_t> host(cape_tables_bytes());
        float* unit = reinterpret_cast<float*>(host.data());
        for (int i = 0; i < 256; ++i) unit[i] = static_cast<uint8_t>(i) / 255.0f;  // as mcrt_build_skin_scene_cape
        uint16_t* map = reinterpret_cast<uint16_t*>(unit + 256);
        for (int i = 0; i < kCapeTexels; ++i) {
            if (pixel[i] < 0 || pixel[i] >= kCapeImageBytes / 4) return nullptr;  // never a read outside the image
            map[i] = static_cast<uint16_t>(pixel[i]);
        }
        void* p = nullptr;
        if (hipMalloc(&p, host.size()) != hipSuccess || hipMemcpy(p, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            if (p) (void)hipFree(p);
            return nullptr;
        }
        t.ptr = p;
    }
    ++t.users;
    return t.ptr;
}
void release_cape_tables(int device) {
    std::lock_guard<std::mutex> lock(g_skin_mutex);
    if (static_cast<size_t>(device) < g_cape_tables.size() && g_cape_tables[static_cast<size_t>(device)].users > 0) --g_cape_tables[static_cast<size_t>(device)].users;
}
namespace {
void free_unused_skin_tables() {  // mcrt_trim
    std::lock_guard<std::mutex> lock(g_skin_mutex);
    for (size_t d = 0; d < g_cape_tables.size(); ++d) {
        SkinTables& t = g_cape_tables[d];
        if (t.ptr && t.users == 0) {
            (void)hipSetDevice(static_cast<int>(d));
            (void)hipFree(t.ptr);
            t.ptr = nullptr;
        }
    }
    for (auto& by_device : g_skin_tables)
        for (size_t d = 0; d < by_device.size(); ++d) {
            SkinTables& t = by_device[d];
            if (t.ptr && t.users == 0) {
                (void)hipSetDevice(static_cast<int>(d));
                (void)hipFree(t.ptr);
                t.ptr = nullptr;
            }
        }
}
}  // namespace

// keeps `s` for reuse unless it is large — MCRT_POOL_MB, by default a twelfth of the device's memory (24 GB of the
// MI355X's 288: the 1080p and 4K frames of BASELINE.json stay pooled, and a host application that never calls
// mcrt_trim() does not sit on a fifth of the card; the one-shot entry points plan their workspace to stay below it, see
// render_to_host) — or the device already has one
size_t pool_limit(int device) {
    static const long long forced_mb = env_ll("MCRT_POOL_MB", -1ll);
    return forced_mb >= 0 ? static_cast<size_t>(forced_mb) << 20 : device_total_memory(device) / 12;
}
namespace {
size_t workspace_bytes(const mcrt_scene* s) {
    size_t n = s->blob.bytes + s->frame.bytes;
    for (const Lane& ln : s->lanes) for_each_buffer(ln, [&](const DeviceBuffer& b) { n += b.bytes; });
    return n;
}

std::mutex g_pool_mutex;
std::vector<mcrt_scene*> g_pool;  // idle scene shells, at most one per device
}  // namespace

bool pool_scene(mcrt_scene* s) {
    const size_t limit = pool_limit(s->device);
    if (workspace_bytes(s) > limit) return false;
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    for (mcrt_scene* q : g_pool)
        if (q->device == s->device) return false;
    g_pool.push_back(s);
    return true;
}
// device < 0: any
mcrt_scene* take_pooled_scene(int device) {
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    for (size_t i = 0; i < g_pool.size(); ++i)
        if (device < 0 || g_pool[i]->device == device) {
            mcrt_scene* s = g_pool[i];
            g_pool.erase(g_pool.begin() + static_cast<long>(i));
            return s;
        }
    return nullptr;
}

void destroy_scene_now(mcrt_scene* s) {
    if (!s) return;
    unregister_live(s);  // before its events go
    if (s->holds_seed_table) g_window_tables.release(s->device);
    if (s->holds_full_table) g_full_tables.release(s->device);
    if (s->holds_sample_table) g_sample_tables.release(s->device);
    if (s->skin_tables) release_skin_tables(s->device, s->skin_height, s->skin_model);
    if (s->cape_tables) release_cape_tables(s->device);
    release_plates(s);
    s->blob.release();  // the other buffers are released by their destructors below
    for (auto& ln : s->lanes) {
        if (ln.stream) (void)hipStreamSynchronize(ln.stream);
        if (ln.done) (void)hipEventDestroy(ln.done);
        if (ln.stream) (void)hipStreamDestroy(ln.stream);
    }
    for (auto& r : s->recorded) {
        if (r.exec) (void)hipGraphExecDestroy(r.exec);
        if (r.graph) (void)hipGraphDestroy(r.graph);
    }
    if (s->capture_stream) (void)hipStreamDestroy(s->capture_stream);
    if (s->fork) (void)hipEventDestroy(s->fork);
    if (s->last_done) (void)hipEventDestroy(s->last_done);
    if (s->staging) (void)hipHostFree(s->staging);
    if (s->main_stream) (void)hipStreamDestroy(s->main_stream);
    if (s->copy_stream) (void)hipStreamDestroy(s->copy_stream);
    for (hipEvent_t m : s->marks) (void)hipEventDestroy(m);
    for (auto& e : s->ev)
        if (e) (void)hipEventDestroy(e);
    delete s;
}

// The parameter tables of the batched launches, per device: a ring of slots, each a device buffer, its pinned host
// staging and an event recorded behind the launches that read it.  A slot is refilled only after that event: a table
// is never overwritten while an earlier batch — on any stream — may still read it.
struct TableSlot {
    DeviceBuffer dev;
    void* host = nullptr;
    size_t host_bytes = 0;
    hipEvent_t done = nullptr;
    bool used = false;  // `done` has been recorded
    bool busy = false;  // being filled by a thread
};
namespace {
constexpr int kTableSlots = 8;
struct DeviceTables {
    TableSlot slot[kTableSlots];
    int next = 0;
};
std::mutex g_table_mutex;
std::vector<DeviceTables*> g_tables;  // by device; a few hundred KB each, kept for the process

TableSlot* acquire_table_slot(int device) {
    std::lock_guard<std::mutex> lock(g_table_mutex);
    if (g_tables.size() <= static_cast<size_t>(device)) g_tables.resize(static_cast<size_t>(device) + 1, nullptr);
    if (!g_tables[static_cast<size_t>(device)]) g_tables[static_cast<size_t>(device)] = new DeviceTables();
    DeviceTables& t = *g_tables[static_cast<size_t>(device)];
    for (int k = 0; k < kTableSlots; ++k) {
        const int i = (t.next + k) % kTableSlots;
        if (t.slot[i].busy) continue;
        t.slot[i].busy = true;
        t.next = (i + 1) % kTableSlots;
        return &t.slot[i];
    }
    return nullptr;
}
void release_table_slot(TableSlot* s) {
    std::lock_guard<std::mutex> lock(g_table_mutex);
    s->busy = false;
}
}  // namespace

int upload_table(int device, const void* rows, size_t bytes, hipStream_t stream, TableUpload& up) {
    TableSlot* slot = acquire_table_slot(device);
    if (!slot) return fail(MCRT_ERR_HIP, "too many batch calls filling parameter tables at once");
    up.slot = slot;
    if (slot->used) HIP_TRY(hipEventSynchronize(slot->done));  // the last launches that read this slot have finished
    if (!slot->done) HIP_TRY(hipEventCreateWithFlags(&slot->done, hipEventDisableTiming));
    if (slot->host_bytes < bytes) {
        if (slot->host) (void)hipHostFree(slot->host);
        slot->host = nullptr;
        slot->host_bytes = 0;
        HIP_TRY(hipHostMalloc(&slot->host, bytes, hipHostMallocDefault));
        slot->host_bytes = bytes;
    }
    HIP_TRY(slot->dev.reserve(bytes));
    std::memcpy(slot->host, rows, bytes);
    up.dev = slot->dev.ptr;
    up.status = hipMemcpyAsync(slot->dev.ptr, slot->host, bytes, hipMemcpyHostToDevice, stream);
    return MCRT_OK;
}
hipError_t TableUpload::commit(hipStream_t stream) {
    const hipError_t e = hipEventRecord(slot->done, stream);
    if (e == hipSuccess) slot->used = true;
    return e;
}
TableUpload::~TableUpload() {
    if (slot) release_table_slot(slot);
}

}  // namespace mcrt_host

using namespace mcrt_host;

extern "C" {

void mcrt_trim(void) {
    for (;;) {
        mcrt_scene* s = take_pooled_scene(-1);
        if (!s) break;
        (void)hipSetDevice(s->device);
        destroy_scene_now(s);
    }
    g_full_tables.free_unused();
    g_window_tables.free_unused();
    g_sample_tables.free_unused();
    free_unused_skin_tables();
    free_unused_plates();
}

int mcrt_device_tables_info(int device, int which, size_t* bytes, int* builds) {
    if (which != MCRT_TABLE_WINDOW && which != MCRT_TABLE_FULL && which != MCRT_TABLE_SAMPLE) return fail(MCRT_ERR_INVALID, "no such table");
    const SeedTables& store = which == MCRT_TABLE_WINDOW ? g_window_tables : (which == MCRT_TABLE_FULL ? g_full_tables : g_sample_tables);
    std::lock_guard<std::mutex> lock(g_seed_mutex);
    const bool known = device >= 0 && static_cast<size_t>(device) < store.by_device.size();
    if (bytes) *bytes = (known && store.by_device[static_cast<size_t>(device)].ptr) ? store.bytes : 0;
    if (builds) *builds = known ? store.by_device[static_cast<size_t>(device)].builds : 0;
    return MCRT_OK;
}
int mcrt_sample_table_info(int device, size_t* bytes, int* builds) { return mcrt_device_tables_info(device, MCRT_TABLE_SAMPLE, bytes, builds); }
int mcrt_scene_tables(mcrt_scene* s, int* mask) {
    if (!s || !mask) return fail(MCRT_ERR_INVALID, "NULL argument");
    *mask = (s->seed_table ? 1 << MCRT_TABLE_WINDOW : 0) | (s->holds_full_table ? 1 << MCRT_TABLE_FULL : 0) | (s->holds_sample_table ? 1 << MCRT_TABLE_SAMPLE : 0);
    return MCRT_OK;
}
int mcrt_bg_plate_info(int device, int* plates, size_t* bytes, int* builds) { return plate_info(kPlatePixels, device, plates, bytes, builds); }
int mcrt_draw_plate_info(int device, int* plates, size_t* bytes, int* builds) { return plate_info(kPlateDraws, device, plates, bytes, builds); }

}  // extern "C"
