// probes.cpp — the mcrt_probe_* entry points: single routines of the kernels run on arrays, for the tests and tools that
// hold the device's arithmetic, intersections and random streams against the reference.
#include "host_internal.h"
#include "mcrt_detmath.h"

#include <cmath>
#include <thread>

using namespace mcrt;
using namespace mcrt_host;

namespace {
// the end of an array probe: the launch's result, then the download of its output; `what` names the probe in the error
int finish_probe(hipError_t launched, void* out, const DeviceBuffer& d_out, size_t bytes, const char* what) {
    hipError_t e = launched;
    if (e == hipSuccess) e = hipMemcpy(out, d_out.ptr, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, what);
    return MCRT_OK;
}
}  // namespace

extern "C" {

int mcrt_probe_intersect(mcrt_scene* s, const float* rays, int n, mcrt_hit* out) {
    if (!s || !rays || !out || n < 0) return fail(MCRT_ERR_INVALID, "bad argument");
    if (n == 0) return MCRT_OK;
    HIP_TRY(hipSetDevice(s->device));
    DeviceBuffer d_rays, d_out;
    HIP_TRY(d_rays.reserve(static_cast<size_t>(n) * 24));
    HIP_TRY(d_out.reserve(static_cast<size_t>(n) * sizeof(mcrt_hit)));
    HIP_TRY(hipMemcpy(d_rays.ptr, rays, static_cast<size_t>(n) * 24, hipMemcpyHostToDevice));
    hipError_t e = launch_probe_intersect(static_cast<const uint8_t*>(s->blob.ptr), static_cast<float*>(d_rays.ptr), n,
                                          static_cast<mcrt_hit*>(d_out.ptr), nullptr);
    return finish_probe(e, out, d_out, static_cast<size_t>(n) * sizeof(mcrt_hit), "probe_intersect");
}

int mcrt_probe_scene_blob(mcrt_scene* s, void* out, size_t capacity) {
    if (!s || !out) return fail(MCRT_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());  // renders and repaints of the handle, on whatever streams
    if (s->host_meshes.size() < sizeof(FlatHeader) || !s->blob.ptr) return fail(MCRT_ERR_INVALID, "the handle holds no scene");
    const size_t bytes = reinterpret_cast<const FlatHeader*>(s->host_meshes.data())->blob_bytes;
    HIP_TRY(hipMemcpy(out, s->blob.ptr, bytes < capacity ? bytes : capacity, hipMemcpyDeviceToHost));
    return static_cast<int>(bytes);
}

int mcrt_probe_units(mcrt_scene* s, uint32_t* records, uint32_t* hits, int capacity) {
    if (!s || capacity < 0) return fail(MCRT_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());  // the handle's renders, on whatever streams
    const Lane& ln = s->lanes[0];
    if (!ln.counters.ptr || !ln.units.ptr || !ln.unit_hits.ptr) return 0;  // nothing rendered yet
    uint32_t n_units = 0;  // frame_info[0]: what `primary` left for `resolve`
    HIP_TRY(hipMemcpy(&n_units, static_cast<const uint32_t*>(ln.counters.ptr) + 2 * kCounterWords, 4, hipMemcpyDeviceToHost));
    if (n_units > 0x7fffffffu || static_cast<size_t>(n_units) * 16 > ln.units.bytes) return fail(MCRT_ERR_INVALID, "the lane's unit count does not fit its workspace");
    const size_t n = n_units < static_cast<uint32_t>(capacity) ? n_units : static_cast<size_t>(capacity);
    if (records && n) HIP_TRY(hipMemcpy(records, ln.units.ptr, n * 16, hipMemcpyDeviceToHost));
    if (hits && n) HIP_TRY(hipMemcpy(hits, ln.unit_hits.ptr, n * 4, hipMemcpyDeviceToHost));
    return static_cast<int>(n_units);
}

int mcrt_probe_trace(mcrt_scene* s, const mcrt_config* cfg, const float* rays, int n, int depth, float* out_rgba) {
    if (!s || !cfg || !rays || !out_rgba || n < 0) return fail(MCRT_ERR_INVALID, "bad argument");
    if (n == 0) return MCRT_OK;
    HIP_TRY(hipSetDevice(s->device));
    DeviceBuffer d_rays, d_out, d_rng, d_stack;
    HIP_TRY(d_rays.reserve(static_cast<size_t>(n) * 24));
    HIP_TRY(d_out.reserve(static_cast<size_t>(n) * 16));
    bool long_rng = (cfg->soft_shadows && 2 * cfg->shadow_samples > 227) || (cfg->ao_enabled && 2 * cfg->ao_samples > 227);
    if (long_rng) HIP_TRY(d_rng.reserve(static_cast<size_t>(n) * 624 * 4));
    if (cfg->max_bounces > 16) HIP_TRY(d_stack.reserve(static_cast<size_t>(n) * cfg->max_bounces * 16));
    HIP_TRY(hipMemcpy(d_rays.ptr, rays, static_cast<size_t>(n) * 24, hipMemcpyHostToDevice));
    hipError_t e = launch_probe_trace(static_cast<const uint8_t*>(s->blob.ptr), *cfg, static_cast<float*>(d_rays.ptr), n,
                                      depth, static_cast<float*>(d_out.ptr), static_cast<uint32_t*>(d_rng.ptr),
                                      static_cast<float*>(d_stack.ptr), nullptr);
    return finish_probe(e, out_rgba, d_out, static_cast<size_t>(n) * 16, "probe_trace");
}

int mcrt_probe_mt_uniform(int device, const uint32_t* seeds, int n_seeds, int n_draws, float* out) {
    if (!seeds || !out || n_seeds < 0 || n_draws < 0) return fail(MCRT_ERR_INVALID, "bad argument");
    if (n_seeds == 0 || n_draws == 0) return MCRT_OK;
    if (mcrt_device_count() <= 0) return fail(MCRT_ERR_NO_DEVICE, "no HIP device");
    HIP_TRY(hipSetDevice(device));
    DeviceBuffer d_seeds, d_out, d_store;
    HIP_TRY(d_seeds.reserve(static_cast<size_t>(n_seeds) * 4));
    HIP_TRY(d_out.reserve(static_cast<size_t>(n_seeds) * n_draws * 4));
    if (n_draws > 227) HIP_TRY(d_store.reserve(static_cast<size_t>(n_seeds) * 624 * 4));
    HIP_TRY(hipMemcpy(d_seeds.ptr, seeds, static_cast<size_t>(n_seeds) * 4, hipMemcpyHostToDevice));
    hipError_t e = launch_probe_mt(static_cast<uint32_t*>(d_seeds.ptr), n_seeds, n_draws, static_cast<float*>(d_out.ptr),
                                   static_cast<uint32_t*>(d_store.ptr), nullptr);
    return finish_probe(e, out, d_out, static_cast<size_t>(n_seeds) * n_draws * 4, "probe_mt");
}

int mcrt_probe_sample_rows(int device, const int32_t* seeds, int n, float* out) {
    if (!seeds || !out || n < 0) return fail(MCRT_ERR_INVALID, "bad argument");
    for (int i = 0; i < n; ++i)
        if (static_cast<uint32_t>(seeds[i]) + kSampleWindowHalf >= kSampleWindow) return fail(MCRT_ERR_INVALID, "seed outside the sample table's window");
    if (n == 0) return MCRT_OK;
    if (mcrt_device_count() <= 0) return fail(MCRT_ERR_NO_DEVICE, "no HIP device");
    HIP_TRY(hipSetDevice(device));
    if (!copy_sample_rows(device, seeds, n, out)) return fail(MCRT_ERR_HIP, "the device has no sample table");
    return MCRT_OK;
}

int mcrt_probe_seed_words(int device, int which, const uint32_t* seeds, int n, uint32_t* out) {
    if (!seeds || !out || n < 0 || (which != MCRT_TABLE_WINDOW && which != MCRT_TABLE_FULL)) return fail(MCRT_ERR_INVALID, "bad argument");
    if (which == MCRT_TABLE_WINDOW)
        for (int i = 0; i < n; ++i)
            if (seeds[i] + kSeedWindowHalf >= kSeedWindow) return fail(MCRT_ERR_INVALID, "seed outside the seed table's window");
    if (n == 0) return MCRT_OK;
    if (mcrt_device_count() <= 0) return fail(MCRT_ERR_NO_DEVICE, "no HIP device");
    HIP_TRY(hipSetDevice(device));
    if (!copy_seed_words(device, which, seeds, n, out)) return fail(MCRT_ERR_HIP, "the device has no such seed table");
    return MCRT_OK;
}

int mcrt_probe_detmath(int device, int op, const float* x, const float* y, size_t n, float* out) {
    if (!x || !out || op < 0 || op > 5 || (op == 2 && !y)) return fail(MCRT_ERR_INVALID, "bad argument");
    if (n == 0) return MCRT_OK;
    if (mcrt_device_count() <= 0) return fail(MCRT_ERR_NO_DEVICE, "no HIP device");
    HIP_TRY(hipSetDevice(device));
    DeviceBuffer dx, dy, dout;
    HIP_TRY(dx.reserve(n * 4));
    HIP_TRY(dout.reserve(n * 4));
    HIP_TRY(hipMemcpy(dx.ptr, x, n * 4, hipMemcpyHostToDevice));
    if (y) {
        HIP_TRY(dy.reserve(n * 4));
        HIP_TRY(hipMemcpy(dy.ptr, y, n * 4, hipMemcpyHostToDevice));
    }
    hipError_t e = launch_probe_detmath(op, static_cast<float*>(dx.ptr), static_cast<float*>(dy.ptr), n,
                                        static_cast<float*>(dout.ptr), nullptr);
    return finish_probe(e, out, dout, n * 4, "probe_detmath");
}

int mcrt_probe_div_const(int device, uint32_t d_first, uint32_t d_count, int mode, uint64_t* mismatches, uint32_t* a_failing_divisor) {
    if (!mismatches || d_first == 0 || d_count == 0 || d_count > 65535u) return fail(MCRT_ERR_INVALID, "bad argument");
    if (mcrt_device_count() <= 0) return fail(MCRT_ERR_NO_DEVICE, "no HIP device");
    HIP_TRY(hipSetDevice(device));
    DeviceBuffer counts, rds;
    HIP_TRY(counts.reserve(16));
    HIP_TRY(rds.reserve(static_cast<size_t>(d_count) * 4));
    {  // the reciprocals as the host forms them for the render kernels (prepare(): 1.0f / float(width))
        std::vector<float> host(d_count);
        for (uint32_t i = 0; i < d_count; ++i) host[i] = 1.0f / static_cast<float>(d_first + i);
        HIP_TRY(hipMemcpy(rds.ptr, host.data(), host.size() * 4, hipMemcpyHostToDevice));
    }
    hipError_t e = hipMemset(counts.ptr, 0, 16);
    for (uint32_t off = 0; e == hipSuccess && off < d_count; off += 32) {  // ~12 G quotients per launch
        e = launch_probe_div_const(d_first + off, d_count - off < 32u ? d_count - off : 32u, mode, static_cast<const float*>(rds.ptr) + off,
                                   static_cast<unsigned long long*>(counts.ptr), nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    unsigned long long host[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpy(host, counts.ptr, 16, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "probe_div_const");
    *mismatches = host[0];
    if (a_failing_divisor) *a_failing_divisor = static_cast<uint32_t>(host[1]);
    return MCRT_OK;
}

int mcrt_probe_detmath_range(int device, int op, uint32_t lo_bits, uint32_t hi_bits, float y0, uint64_t* mismatches) {
    if (!mismatches || op < 0 || op > 5 || hi_bits < lo_bits) return fail(MCRT_ERR_INVALID, "bad argument");
    if (mcrt_device_count() <= 0) return fail(MCRT_ERR_NO_DEVICE, "no HIP device");
    HIP_TRY(hipSetDevice(device));
    const uint64_t total = static_cast<uint64_t>(hi_bits) - lo_bits + 1;
    const uint64_t chunk = 1ull << 26;  // 64 Mi values = 256 MiB per pass
    DeviceBuffer dout;
    HIP_TRY(dout.reserve(chunk * 4));
    std::vector<float> host(chunk);
    unsigned nt = std::thread::hardware_concurrency();
    if (nt == 0) nt = 4;
    if (nt > 32) nt = 32;
    uint64_t bad = 0;
    for (uint64_t off = 0; off < total; off += chunk) {
        uint64_t cnt = total - off < chunk ? total - off : chunk;
        uint32_t base = lo_bits + static_cast<uint32_t>(off);
        hipError_t e = launch_probe_detmath_range(op, base, cnt, y0, static_cast<float*>(dout.ptr), nullptr);
        if (e == hipSuccess) e = hipMemcpy(host.data(), dout.ptr, cnt * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(e, "probe_detmath_range");
        std::atomic<uint64_t> part{0};
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < nt; ++t)
            pool.emplace_back([&, t] {
                uint64_t b = 0;
                for (uint64_t i = t; i < cnt; i += nt) {
                    float x = mcrt_u2f(base + static_cast<uint32_t>(i));
                    // ops 3/4 (device: the fused mcrt_sincosf) are held against the separate functions
                    float ref = op == 5 ? 1.0f / x
                                        : ((op == 0 || op == 3) ? mcrt_sinf(x) : ((op == 1 || op == 4) ? mcrt_cosf(x) : mcrt_powf(x, y0)));
                    uint32_t a = mcrt_f2u(ref), d = mcrt_f2u(host[i]);
                    if (a != d && !(std::isnan(ref) && std::isnan(host[i]))) ++b;
                }
                part += b;
            });
        for (auto& th : pool) th.join();
        bad += part.load();
    }
    *mismatches = bad;
    return MCRT_OK;
}

}  // extern "C"
