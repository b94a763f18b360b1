// util_kernels.hip — small kernels beside the renderer: unpacking and assembling sharded frames, RGBA8 quantisation, the
// devices' seed tables, and the probes the test suites call (probes.cpp).
#include "kernel_common.h"

namespace mcrt {

using namespace rt;

template <class Pixel>  // float4, or uchar4 for the RGBA8 plane
__global__ void unpack_rows_kernel(mcrt_config cfg, Shard sh, const Pixel* packed, Pixel* frame) {
    // one thread per packed pixel
    size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    int W = cfg.width, T = cfg.tile_size;
    size_t prow = i / W;
    int x = static_cast<int>(i - prow * W);
    int k = static_cast<int>(prow / T);
    int ly = static_cast<int>(prow - static_cast<size_t>(k) * T);
    if (k >= sh.owned_rows) return;
    int y = (sh.first + k * sh.step) * T + ly;
    if (y >= cfg.height) return;
    frame[static_cast<size_t>(y) * W + x] = packed[i];
}

// every rank's packed rows (rank-major, `rank_stride` float4 apart) → the frame, one thread per output
// pixel: tile row r belongs to rank r mod world and is that rank's (r div world)-th packed tile row
__global__ void assemble_frame_kernel(mcrt_config cfg, int world, const float4* __restrict__ gathered, size_t rank_stride,
                                      float4* __restrict__ frame) {
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int W = cfg.width, T = cfg.tile_size;
    if (i >= static_cast<size_t>(W) * cfg.height) return;
    const int y = static_cast<int>(i / W);
    const int x = static_cast<int>(i - static_cast<size_t>(y) * W);
    const int r = y / T, ly = y - r * T;
    const int rank = r % world, k = r / world;
    frame[i] = gathered[static_cast<size_t>(rank) * rank_stride + (static_cast<size_t>(k) * T + ly) * W + x];
}

// the device's seed table (kernels.h): entry i = mt[397] of std::mt19937(i - kSeedWindowHalf)
__global__ __launch_bounds__(256) void seed_table_kernel(uint32_t* __restrict__ table) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < kSeedWindow) table[i] = MtShort::word397(i - kSeedWindowHalf);
}

// the full table: entry s = mt[397] of std::mt19937(s), for the seeds first + (this thread)
__global__ __launch_bounds__(256) void seed_table_range_kernel(uint32_t* __restrict__ table, uint32_t first) {
    const uint32_t s = first + blockIdx.x * 256u + threadIdx.x;
    table[s] = MtShort::word397(s);
}

// the device's sample table (kernels.h): row r = the kSampleRow elements of seed r - kSampleWindowHalf, a thread per row, by the
// engine and the routines disk_sample_positions runs (the 397-step seeding recurrence per row: 3.3 G steps in all, well under a millisecond)
__global__ __launch_bounds__(256) void sample_table_kernel(float4* __restrict__ table) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= kSampleWindow) return;
    MtShort rng;
    rng.seed(r - kSampleWindowHalf);
    float4* __restrict__ row = table + static_cast<size_t>(r) * kSampleRow;
    for (int i = 0; i < kSampleRow; ++i) {
        const float d0 = rng.uniform();
        const float d1 = rng.uniform();
        row[i] = sample_row_element(d0, d1);
    }
}

__global__ void quantize_kernel(const float4* rgba, uchar4* out, size_t n) {  // image_writer.cpp:18-22
    size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = quantize_pixel(rgba[i]);
}

__global__ void probe_intersect_kernel(const uint8_t* scene, const float* rays, int n, mcrt_hit* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    SceneView sc = view_of(scene);
    Ray r{ld3(rays + 6 * i), ld3(rays + 6 * i + 3)};
    Hit h = hit_scene(sc, r, ~0ull);
    mcrt_hit o;
    o.hit = h.hit ? 1 : 0;
    o.t = h.t;
    o.point[0] = h.p.x, o.point[1] = h.p.y, o.point[2] = h.p.z;
    o.normal[0] = h.n.x, o.normal[1] = h.n.y, o.normal[2] = h.n.z;
    o.texture_color[0] = h.tex.r, o.texture_color[1] = h.tex.g, o.texture_color[2] = h.tex.b,
    o.texture_color[3] = h.tex.a;
    o.is_outer_layer = h.outer ? 1 : 0;
    out[i] = o;
}

__global__ void probe_trace_kernel(const uint8_t* scene, mcrt_config cfg, const float* rays, int n, int depth,
                                   float* out, uint32_t* hit_rng, float* deep_stack) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    SceneView sc = view_of(scene);
    Ray r{ld3(rays + 6 * i), ld3(rays + 6 * i + 3)};
    C4 local_stack[kMaxStack];
    C4* stack = deep_stack ? reinterpret_cast<C4*>(deep_stack) + static_cast<size_t>(i) * max(cfg.max_bounces, 1)
                           : local_stack;
    uint32_t* rng = hit_rng ? hit_rng + static_cast<size_t>(i) * 624 : nullptr;
    C4 c;
    if (depth > cfg.max_bounces) {
        c = background(sc, cfg, 0.5f, 0.5f);
    } else {
        Hit h = hit_scene(sc, r, ~0ull);
        if (!h.hit) {
            const float* b = sc.hdr->background;
            c = (depth == 0) ? background(sc, cfg, 0.5f, 0.5f) : C4{b[0], b[1], b[2], b[3]};
        } else {
            c = trace_from_hit(sc, cfg, r, h, depth, stack, rng);
        }
    }
    out[4 * i + 0] = c.r, out[4 * i + 1] = c.g, out[4 * i + 2] = c.b, out[4 * i + 3] = c.a;
}

__global__ void probe_mt_kernel(const uint32_t* seeds, int n_seeds, int n_draws, float* out, uint32_t* storage) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_seeds) return;
    HitRng g;
    g.seed(seeds[i], n_draws, storage ? storage + static_cast<size_t>(i) * 624 : nullptr);
    for (int k = 0; k < n_draws; ++k) out[static_cast<size_t>(i) * n_draws + k] = g.uniform();
}

__device__ __forceinline__ float detmath_op(int op, float x, float y) {
    if (op == 3 || op == 4) {  // the fused form: .s / .c
        float sn, cs;
        mcrt_sincosf(x, &sn, &cs);
        return op == 3 ? sn : cs;
    }
    if (op == 5) return rcp_exact(x);  // held against the host's IEEE 1.0f / x
    return op == 0 ? mcrt_sinf(x) : (op == 1 ? mcrt_cosf(x) : mcrt_powf(x, y));
}
__global__ void probe_detmath_kernel(int op, const float* x, const float* y, size_t n, float* out) {
    size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = detmath_op(op, x[i], y ? y[i] : 0.0f);
}
__global__ void probe_detmath_range_kernel(int op, uint32_t lo_bits, uint64_t count, float y0, float* out) {
    uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= count) return;
    out[i] = detmath_op(op, mcrt_u2f(lo_bits + static_cast<uint32_t>(i)), y0);
}

// div_frame against the general division for the divisors d_first .. d_first + gridDim.y - 1 and every float x in
// {0} and [2^-33, d + 1] (by bit pattern).  counts[0] += mismatches, counts[1] = a failing divisor
// rds: the divisors' reciprocals as the HOST forms them (what the render kernels are given: RenderParams::inv_width / inv_height)
__global__ void probe_div_const_kernel(uint32_t d_first, int mode, const float* __restrict__ rds, unsigned long long* counts) {
    const float d = static_cast<float>(d_first + blockIdx.y);
    const float rd = rds[blockIdx.y];
    if (mode == 4) {  // the device's own 1.0f / d against the host's reciprocal
        if (blockIdx.x == 0 && threadIdx.x == 0 && __float_as_uint(1.0f / d) != __float_as_uint(rd)) {
            atomicAdd(&counts[0], 1ull);
            counts[1] = d_first + blockIdx.y;
        }
        return;
    }
    if (mode == 3) {  // rt::sqrt_pos against sqrtf for 0 and every float from 2^-96 to infinity (the divisor plays no part)
        unsigned long long bad = 0;
        const uint32_t lo = 0x0f800000u /* 2^-96 */, hi = 0x7f800000u;
        for (uint64_t b = static_cast<uint64_t>(lo) + static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; b <= hi + 1ull;
             b += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
            const float x = b > hi ? 0.0f : __uint_as_float(static_cast<uint32_t>(b));
            if (__float_as_uint(__builtin_sqrtf(x)) != __float_as_uint(sqrt_pos(x))) ++bad;
        }
        if (bad) atomicAdd(&counts[0], bad);
        return;
    }
    const uint32_t lo = 0x2f000000u /* 2^-33 */, hi = __float_as_uint(d + 1.0f);
    unsigned long long bad = 0;
    for (uint64_t b = static_cast<uint64_t>(lo) + static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; b <= hi + 1ull;
         b += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const float x = b > hi ? 0.0f : __uint_as_float(static_cast<uint32_t>(b));
        const float want = x / d;
        const float got = mode == 2 ? x * rd : (mode ? div_frame2(x, d, rd) : div_frame(x, d, rd));  // mode 1: two corrections; mode 2: none (the probe's own check)
        if (__float_as_uint(want) != __float_as_uint(got)) ++bad;
    }
    if (bad) {
        atomicAdd(&counts[0], bad);
        counts[1] = d_first + blockIdx.y;
    }
}

// ---- host-side launchers ------------------------------------------------------------------------
// a thread per item in blocks of kThreads; nothing to launch for n <= 0
template <int kThreads, class Kernel, class N, class... Args>
static hipError_t launch_flat(Kernel kernel, N n, hipStream_t stream, Args... args) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>((static_cast<size_t>(n) + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, args...);
    return hipGetLastError();
}

hipError_t launch_unpack_rows(const mcrt_config& cfg, const Shard& sh, const float* packed, float* frame, hipStream_t stream) {
    const size_t n = static_cast<size_t>(sh.owned_rows) * cfg.tile_size * cfg.width;
    return launch_flat<256>(unpack_rows_kernel<float4>, n, stream, cfg, sh, reinterpret_cast<const float4*>(packed), reinterpret_cast<float4*>(frame));
}
hipError_t launch_unpack_rows8(const mcrt_config& cfg, const Shard& sh, const uint8_t* packed, uint8_t* frame, hipStream_t stream) {
    const size_t n = static_cast<size_t>(sh.owned_rows) * cfg.tile_size * cfg.width;
    return launch_flat<256>(unpack_rows_kernel<uchar4>, n, stream, cfg, sh, reinterpret_cast<const uchar4*>(packed), reinterpret_cast<uchar4*>(frame));
}
hipError_t launch_assemble_frame(const mcrt_config& cfg, int world, const float* gathered, size_t rank_stride_pixels, float* frame, hipStream_t stream) {
    const size_t n = static_cast<size_t>(cfg.width) * cfg.height;
    return launch_flat<256>(assemble_frame_kernel, n, stream, cfg, world, reinterpret_cast<const float4*>(gathered), rank_stride_pixels, reinterpret_cast<float4*>(frame));
}
hipError_t launch_quantize(const float* rgba, uint8_t* out, size_t n_pixels, hipStream_t stream) {
    return launch_flat<256>(quantize_kernel, n_pixels, stream, reinterpret_cast<const float4*>(rgba), reinterpret_cast<uchar4*>(out), n_pixels);
}

hipError_t launch_build_seed_table(uint32_t* table, hipStream_t stream) { return launch_flat<256>(seed_table_kernel, kSeedWindow, stream, table); }
hipError_t launch_build_seed_table_range(uint32_t* table, uint32_t first, uint32_t count, hipStream_t stream) {
    if (count == 0u || (count & 255u)) return hipErrorInvalidValue;
    return launch_flat<256>(seed_table_range_kernel, count, stream, table, first);
}

hipError_t launch_build_sample_table(float4* table, hipStream_t stream) { return launch_flat<256>(sample_table_kernel, kSampleWindow, stream, table); }

hipError_t launch_probe_div_const(uint32_t d_first, uint32_t d_count, int mode, const float* host_reciprocals, unsigned long long* counts, hipStream_t stream) {
    if (d_count == 0) return hipSuccess;
    hipLaunchKernelGGL(probe_div_const_kernel, dim3(mode == 4 ? 1 : 2048, d_count), dim3(256), 0, stream, d_first, mode, host_reciprocals, counts);
    return hipGetLastError();
}
hipError_t launch_probe_intersect(const uint8_t* scene, const float* rays, int n, mcrt_hit* out, hipStream_t stream) {
    return launch_flat<64>(probe_intersect_kernel, n, stream, scene, rays, n, out);
}
hipError_t launch_probe_trace(const uint8_t* scene, const mcrt_config& cfg, const float* rays, int n, int depth, float* out, uint32_t* hit_rng, float* deep_stack,
                              hipStream_t stream) {
    return launch_flat<64>(probe_trace_kernel, n, stream, scene, cfg, rays, n, depth, out, hit_rng, deep_stack);
}
hipError_t launch_probe_mt(const uint32_t* seeds, int n_seeds, int n_draws, float* out, uint32_t* storage, hipStream_t stream) {
    return launch_flat<64>(probe_mt_kernel, n_seeds, stream, seeds, n_seeds, n_draws, out, storage);
}
hipError_t launch_probe_detmath(int op, const float* x, const float* y, size_t n, float* out, hipStream_t stream) {
    return launch_flat<256>(probe_detmath_kernel, n, stream, op, x, y, n, out);
}
hipError_t launch_probe_detmath_range(int op, uint32_t lo_bits, uint64_t count, float y0, float* out, hipStream_t stream) {
    return launch_flat<256>(probe_detmath_range_kernel, count, stream, op, lo_bits, count, y0, out);
}

}  // namespace mcrt
