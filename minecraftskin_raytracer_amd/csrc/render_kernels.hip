// render_kernels.hip — the render pipeline: hand-written HIP kernels for gfx950 (MI355X / CDNA4) and their launchers.
//
// The hot path of the reference, TileRenderer::renderTile (tile_renderer.cpp:71-127) with
// RayTracer::traceRay underneath, as a wavefront pipeline: every stage is a small, high-occupancy
// kernel over a dense work list, so the latency-bound pieces (the 397-step mt19937 seeding chain,
// the dependent slab tests of a shadow ray) are hidden by many resident waves instead of stalling a
// workgroup, and hit work is spread over the whole chip no matter which tiles hold the character.
//
//   seed_tiles      1 lane / tile     mt19937 seeding of the per-tile jitter streams (kept across renders: the
//                                     seeds depend on the frame width, the tile size and the shard only)
//   plan_tiles      1 wave / tile     which meshes' screen bounds touch the tile (a tile nothing can touch
//                                     is rendered whole as background; others are split into pixel-aligned
//                                     units with colour slots assigned), then every draw of the tile's
//                                     mt19937 stream — twisted inside the wave, no workgroup barrier — to HBM
//   primary         persistent WGs    touched units: thread per sample, its draws, camera/lens ray, closest
//                                     hit over the tile's mesh mask; misses write their sample colour, hits
//                                     become records at the front of the unit's slot range.  (Background tiles only when
//                                     a pixel takes more than 24 draws: thread per pixel, gradient, ordered sample sum)
//                                     ... and, packed on the block's first threads, the reflection ray of every
//                                     primary hit (geometry only: direction, hit point, normal) → closest hit →
//                                     level-1 record; chains that end are marked
//   ... then ONCE over the records of ALL levels (320 k + 31 k + 3 k + ... at 1080p / 4 spp):
//   ao              (AO on) 1 lane / primary hit   the meshes its hemisphere of rays can meet; mt19937(ao seed), the A
//                                     cosine-weighted directions and their any-hit tests within the radius, in registers
//   lit             first, per block of 256 level-1 records (1 lane / record): the rest of the chain — reflect, closest
//                                     hit, append, until the ray misses or maxBounces is reached (~10 % go on per level) —
//                                     into a region of the queue the block owns, lit and shaded by the same workgroup;
//                   then phases per block of 256 records, handed over through LDS:
//                   1 lane / record   the hit's bundle mask (meshes its shadow rays can meet) and the whole-bundle
//                                     decision (rt::bundle_classify): most hits are provably lit by all S light
//                                     samples or by none and need no samples and no rays; the rest are packed
//                   1 lane / undecided record   register-only truncated mt19937 → 2·S draws → the S disk sample positions
//                   1 lane / (undecided record, light sample)   exact any-hit test on the meshes left open → lit count
//                   1 lane / record   Blinn-Phong (+AO) → the chain's stack of level colours
//   resolve         1 lane / pixel    folds each sample's chain back to front, ordered sum of the pixel's sample
//                                     colours (float addition order is part of the result), coalesced float4 / RGBA8 store
//                                     (transparent background: `plan_tiles` fills background tiles with (0,0,0,0), and
//                                     `resolve_transparent` sums the samples that hit only — mcrt.h)
//   (general variants — per-hit RNG streams longer than 227 draws, or more than kFlatMaxBounces bounces — run
//   light_samples / shadow / level_shade once per recursion level instead of lit, and `primary` traces no
//   reflection rays)
// Records live in HBM as SoA float4 arrays.  Every unit owns a fixed slot range (its samples); its
// primary hits are compacted to the front of that range with an LDS prefix sum and a per-unit count —
// NO global atomics on the hot path (a returning atomic on one word sustains only ~88 ops/us on this
// chip; per-wave queue claims made `primary` atomic-bound); deeper records take one atomic per 256.
// A frame is cut into batches of tile rows so that the worst case (every sample of a touched tile hits) fits.
// No MFMA: there is no dense contraction anywhere on this path.
// Beside this file: the stand-alone passes (layers and picks, ground shadow, skin repaints) in pass_kernels.hip, the small
// kernels and the probes in util_kernels.hip, what the kernel files share in kernel_common.h, and the host planning that
// sizes every launch here (workspace, batches, grids, plates) in render_plan.cpp.
#include "kernel_common.h"

namespace mcrt {

using namespace rt;

// (px + jitter) / width and (py + jitter) / height of a sample (tile_renderer.cpp:88-89): rt::div_frame where the
// frame's size lies in its verified range, the general division otherwise
struct FrameDiv {
    float w, h, rw, rh;
    bool fast;
    __device__ __forceinline__ explicit FrameDiv(const RenderParams& p)
        : w(static_cast<float>(p.cfg.width)), h(static_cast<float>(p.cfg.height)), rw(p.inv_width), rh(p.inv_height), fast(p.div_frame != 0) {}
    // with the frame's size as floats already at hand (`resolve` forms them once per kernel)
    __device__ __forceinline__ FrameDiv(float fw, float fh, const RenderParams& p) : w(fw), h(fh), rw(p.inv_width), rh(p.inv_height), fast(p.div_frame != 0) {}
    __device__ __forceinline__ float u(float x) const { return fast ? div_frame(x, w, rw) : x / w; }
    __device__ __forceinline__ float v(float y) const { return fast ? div_frame(y, h, rh) : y / h; }
};

// A wave-uniform float that a kernel forms once and keeps across its item loop, in a scalar register: conversions and
// divisions run on the vector unit, and their result would otherwise hold a VGPR — or be formed again by every phase.
// (`resolve`, which has registers to spare.  In `primary` the three scalars cost more lane moves than they saved.)
__device__ __forceinline__ float uniform_float(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }

__device__ __forceinline__ TileGeom tile_of(const RenderParams& p, int owned_tile) {
    TileGeom t;
    if (p.rect_w > 0) {  // the one tile of a renderTile call: any rectangle of the frame
        t.x = p.rect_x, t.y = p.rect_y, t.w = p.rect_w, t.h = p.rect_h;
        t.owned_row = 0;
        t.frame_tile = 0;
        return t;
    }
    int k = owned_tile / p.shard.tiles_x;
    int tx = owned_tile - k * p.shard.tiles_x;
    int ty = p.shard.first + k * p.shard.step;
    int ts = p.cfg.tile_size;
    t.x = tx * ts;
    t.y = ty * ts;
    t.w = min(ts, p.cfg.width - t.x);
    t.h = min(ts, p.cfg.height - t.y);
    t.owned_row = k;
    t.frame_tile = ty * p.shard.tiles_x + tx;
    return t;
}

// ---------------------------------------------------------------------------------------------
// pre-pass: seed one std::mt19937 per owned tile (tile_renderer.cpp:78).  The seeding
// recurrence is strictly sequential, so it is spread over lanes (one tile per lane).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void seed_tiles_body(const RenderParams& __restrict__ p, int n_tiles) {
    int tile = blockIdx.x * 64 + threadIdx.x;
    if (tile >= n_tiles) return;
    TileGeom t = tile_of(p, tile);
    uint32_t x = static_cast<uint32_t>(t.y * p.cfg.width + t.x);
    uint32_t* dst = p.tile_rng + static_cast<size_t>(tile) * p.stream_parts * 624;
    dst[0] = x;
    for (uint32_t j = 1; j < 624; ++j) {
        x = mt_step(x, j);
        dst[j] = x;
    }
}
__global__ __launch_bounds__(64) void seed_tiles_kernel(RenderParams p, int n_tiles) { seed_tiles_body(p, n_tiles); }

// ---------------------------------------------------------------------------------------------
// pixel store: the float4 frame and/or its RGBA8 quantisation `(u8)(clamp(c,0,1)*255+0.5)`
// (image_writer.cpp:18-22 ≡ image.cpp:31-36) — the epilogue of `primary` (background tiles) and `resolve`
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void store_pixel(float4* __restrict__ out_frame, uchar4* __restrict__ out8, size_t idx, float4 v) {
    if (out_frame) out_frame[idx] = v;
    if (out8) out8[idx] = quantize_pixel(v);
}

// ---------------------------------------------------------------------------------------------
// tile_streams: every draw renderTile takes from a tile's mt19937 (tile_renderer.cpp:78-99: per pixel
// in row-major order, per sample, 2 jitter draws if spp > 1, then 2 lens draws if DOF is on).  One
// WAVE per tile: the engine's twist runs inside the wave on a ping-pong state in LDS — LDS
// operations of one wave are ordered, a wave barrier keeps the compiler from moving them — so
// there is no workgroup barrier anywhere and all tiles of a batch advance in parallel.
//  * A tile that meshes can touch: the draws go to HBM as uniform floats, for `primary`.
//  * A background tile (93 % of the tiles of the metric frame): nothing can be hit, no ray is needed —
//    the wave renders the tile itself, straight from the draws in LDS: after each twist the pixels whose
//    draws are complete (they lie in the new 624 words and the previous 624, both still in LDS) get
//    their gradient samples, the ordered sample sum (tile_renderer.cpp:111-124) and a coalesced store.
//    Writing those streams out and reading them back in `primary` was 134 MB of the frame's HBM traffic.
//    Pays while a twist completes enough pixels to fill the wave's lanes (spp * draws per sample <= 24:
//    RenderParams::bg_in_plan); at higher sample counts every tile's stream goes to HBM and `primary`
//    renders the background tiles with a thread per pixel.
// (Generating the stream inside `primary` with block-wide twists made that kernel barrier-bound: 3
// barriers per 624 draws, ~60 us of the 1080p / 4 spp frame, milliseconds at 64 spp.)
// ---------------------------------------------------------------------------------------------
// the pixels [lo, hi) of a background tile; draw(g, jx, jy) = draws number g, g + 1 of the tile's stream (g even)
// kToPlate: out_frame is a background plate (kernels.h) — the pixel goes to the tile's slot, tile-major, instead of the frame
template <bool kToPlate = false, class DrawFn>
__device__ __forceinline__ void background_pixels(const SceneView& sc, const RenderParams& p, const TileGeom& tg, float4* __restrict__ out_frame,
                                                  uchar4* __restrict__ out8, unsigned lo, unsigned hi, int lane, DrawFn&& draw) {
    const mcrt_config& cfg = p.cfg;
    const int spp = cfg.samples_per_pixel > 1 ? cfg.samples_per_pixel : 1;
    const unsigned dd = static_cast<unsigned>(p.draws_per_sample);
    const FrameDiv fd(p);
    const float inv_spp = 1.0f / static_cast<float>(spp);
    const UDiv by_w(static_cast<unsigned>(tg.w));
    for (unsigned pix = lo + static_cast<unsigned>(lane); pix < hi; pix += 64u) {
        const unsigned uly = by_w.div(pix);
        const int ly = static_cast<int>(uly);
        const int lx = static_cast<int>(pix - uly * static_cast<unsigned>(tg.w));
        const float fx = static_cast<float>(tg.x + lx), fy = static_cast<float>(tg.y + ly);
        const unsigned g0 = pix * static_cast<unsigned>(spp) * dd;  // (a tile's stream is shorter than 2^32 draws: plan_workspace)
        float ar = 0.0f, ag = 0.0f, ab = 0.0f, aa = 0.0f;
        for (int sidx = 0; sidx < spp; ++sidx) {
            float jx = 0.5f, jy = 0.5f;
            if (spp > 1) draw(g0 + static_cast<unsigned>(sidx) * dd, jx, jy);  // the sample's two jitter draws: one aligned pair of the stream
            const C4 c = background(sc, cfg, fd.u(fx + jx), fd.v(fy + jy));  // tile_renderer.cpp:111-114
            ar += c.r;
            ag += c.g;
            ab += c.b;
            aa += c.a;
        }
        const float4 pixel = make_float4(ar * inv_spp, ag * inv_spp, ab * inv_spp, aa * inv_spp);
        if constexpr (kToPlate) {
            out_frame[static_cast<size_t>(tg.frame_tile) * static_cast<size_t>(cfg.tile_size) * static_cast<size_t>(cfg.tile_size) + pix] = pixel;
        } else {
            const int row = (p.layout == MCRT_LAYOUT_PACKED) ? ((p.shard.pack_first + tg.owned_row * p.shard.pack_step) * cfg.tile_size + ly) : (tg.y + ly);
            store_pixel(out_frame, out8, static_cast<size_t>(row) * cfg.width + (tg.x + lx), pixel);
        }
    }
}

// A background tile whose every sample has the same colour needs no draws at all: the flat background colour
// (gradient off, raytracer.cpp:32-33), or the gradient's edge colour when the whole tile lies where the reference's
// `dist` clamps to 1 — sqrt(cx² + cy²)·2·gradientScale >= 1 for every point a jittered sample of the tile can take
// (raytracer.cpp:19-24; 18 % of the metric frame's tiles, its corners).  The test uses the tile's rectangle in u,v with a
// margin of 1e-4, a hundred times the float error of the reference's expression; the colour and the sample sum are
// formed by the reference's own operations (c = center·(1 - t) + edge·t with t = 1·1; spp additions; · 1/spp).
__device__ __forceinline__ bool constant_background(const SceneView& sc, const RenderParams& p, const TileGeom& tg, float4& pixel) {
    const mcrt_config& cfg = p.cfg;
    C4 c;
    if (cfg.gradient_bg) {
        const float fW = static_cast<float>(cfg.width), fH = static_cast<float>(cfg.height);
        const float ulo = static_cast<float>(tg.x) / fW, uhi = static_cast<float>(tg.x + tg.w) / fW;
        const float vlo = static_cast<float>(tg.y) / fH, vhi = static_cast<float>(tg.y + tg.h) / fH;
        const float cx = (ulo <= 0.5f && 0.5f <= uhi) ? 0.0f : fminf(fabsf(ulo - 0.5f), fabsf(uhi - 0.5f));
        const float cy = (vlo <= 0.5f && 0.5f <= vhi) ? 0.0f : fminf(fabsf(vlo - 0.5f), fabsf(vhi - 0.5f));
        if (!(__builtin_sqrtf(cx * cx + cy * cy) * 2.0f * cfg.gradient_scale >= 1.0f + 1e-4f)) return false;
        const float dist = 1.0f;  // sclamp(dist, 0, 1)
        const float t = dist * dist;
        c.r = cfg.bg_center[0] * (1.0f - t) + cfg.bg_edge[0] * t;
        c.g = cfg.bg_center[1] * (1.0f - t) + cfg.bg_edge[1] * t;
        c.b = cfg.bg_center[2] * (1.0f - t) + cfg.bg_edge[2] * t;
        c.a = 1.0f;
    } else {
        const float* b = sc.hdr->background;
        c = C4{b[0], b[1], b[2], b[3]};
    }
    const int spp = cfg.samples_per_pixel > 1 ? cfg.samples_per_pixel : 1;
    const float inv_spp = 1.0f / static_cast<float>(spp);
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, aa = 0.0f;
    for (int sidx = 0; sidx < spp; ++sidx) {  // tile_renderer.cpp:116-124
        ar += c.r;
        ag += c.g;
        ab += c.b;
        aa += c.a;
    }
    pixel = make_float4(ar * inv_spp, ag * inv_spp, ab * inv_spp, aa * inv_spp);
    return true;
}
// the tile's pixels get `pixel`; `nthreads` threads (a wave, or a workgroup), this one being number `tid`
__device__ __forceinline__ void fill_tile(const RenderParams& p, const TileGeom& tg, float4* __restrict__ out_frame, uchar4* __restrict__ out8, float4 pixel,
                                          unsigned tid, unsigned nthreads) {
    const unsigned npix = static_cast<unsigned>(tg.w) * static_cast<unsigned>(tg.h);
    const UDiv by_w(static_cast<unsigned>(tg.w));
    for (unsigned pix = tid; pix < npix; pix += nthreads) {
        const unsigned uly = by_w.div(pix);
        const int ly = static_cast<int>(uly);
        const int lx = static_cast<int>(pix - uly * static_cast<unsigned>(tg.w));
        const int row = (p.layout == MCRT_LAYOUT_PACKED) ? ((p.shard.pack_first + tg.owned_row * p.shard.pack_step) * p.cfg.tile_size + ly) : (tg.y + ly);
        store_pixel(out_frame, out8, static_cast<size_t>(row) * p.cfg.width + (tg.x + lx), pixel);
    }
}

// the tile's pixels from its slot of the background plate (kernels.h): one coalesced 16-byte load per pixel, then the
// frame's own store (layout, RGBA8 plane); `nthreads` threads, this one being number `tid`
__device__ __forceinline__ void copy_plate_tile(const RenderParams& p, const TileGeom& tg, float4* __restrict__ out_frame, uchar4* __restrict__ out8,
                                                unsigned tid, unsigned nthreads) {
    const unsigned npix = static_cast<unsigned>(tg.w) * static_cast<unsigned>(tg.h);
    const float4* __restrict__ src = p.bg_plate + static_cast<size_t>(tg.frame_tile) * static_cast<size_t>(p.cfg.tile_size) * static_cast<size_t>(p.cfg.tile_size);
    const UDiv by_w(static_cast<unsigned>(tg.w));
    for (unsigned pix = tid; pix < npix; pix += nthreads) {
        const float4 pixel = src[pix];
        const unsigned uly = by_w.div(pix);
        const int ly = static_cast<int>(uly);
        const int lx = static_cast<int>(pix - uly * static_cast<unsigned>(tg.w));
        const int row = (p.layout == MCRT_LAYOUT_PACKED) ? ((p.shard.pack_first + tg.owned_row * p.shard.pack_step) * p.cfg.tile_size + ly) : (tg.y + ly);
        store_pixel(out_frame, out8, static_cast<size_t>(row) * p.cfg.width + (tg.x + lx), pixel);
    }
}

// executed by one wave; `st` = its 2 x 624 words of LDS.  dst != nullptr: the tile's draws go there;
// dst == nullptr: a background tile, rendered from the draws in LDS.
// jitter_only (a background tile under depth of field, 4 draws per sample): only the samples' jitter pairs are stored,
// packed — sample k's at dst[2k], dst[2k + 1]; no ray leaves a background tile, so its lens draws are never read
// (tile_renderer.cpp:99-114), and they are half of the stream `primary` would read back.
//
// A tile's stream is cut into `stream_parts` PARTS of `stream_part_twists` twists each: the engine's state at the start
// of every part — after 0, q, 2q, ... twists — is a function of the tile's seed alone and is kept with the tile seeds
// (advance_tiles_kernel), so `stream_waves` waves (1, 2 or 4, each taking stream_parts / stream_waves consecutive parts)
// can advance side by side instead of ONE wave running the whole chain of dependent twists (13 at 1080p / 4 spp, 210 at
// 64 spp: `plan_tiles` alone on the device is the latency of that chain at two waves per SIMD).  A wave writes its own
// draws, or — background tile — renders the pixels whose FIRST draw lies in its parts; a pixel whose draws run over their
// end is finished by one more twist of the same wave (the next wave makes the same words again).
template <bool kToPlate = false>
__device__ __forceinline__ void tile_stream_wave(const SceneView& sc, const uint32_t* __restrict__ tile_rng, float* __restrict__ dst,
                                                 float4* __restrict__ out_frame, uchar4* __restrict__ out8, const RenderParams& p,
                                                 const TileGeom& tg, int tile, int part, int n_parts, uint32_t* st, int lane, bool jitter_only = false) {
    const int spp = p.cfg.samples_per_pixel > 1 ? p.cfg.samples_per_pixel : 1;
    const unsigned npix = static_cast<unsigned>(tg.w) * static_cast<unsigned>(tg.h);
    const unsigned per_pixel = static_cast<unsigned>(spp) * static_cast<unsigned>(p.draws_per_sample);
    const unsigned total = npix * per_pixel;  // < 2^32 - 2^16 (plan_workspace refuses longer streams): 32-bit index arithmetic throughout
    // this wave: parts [part, part + n_parts) — it starts from the state kept for `part` and simply twists on through the others
    const unsigned part_draws = static_cast<unsigned>(p.stream_part_twists) * 624u;
    const unsigned first_draw = static_cast<unsigned>(part) * part_draws;  // (parts x part_draws covers a full tile's stream: no overflow)
    if (first_draw >= total) return;  // a clipped tile's stream ends before this part
    const unsigned wave_draws = static_cast<unsigned>(n_parts) * part_draws;
    const bool last_part = part + n_parts >= p.stream_parts || first_draw + wave_draws >= total;
    const unsigned end_draw = last_part ? total : first_draw + wave_draws;
    // background tile: the pixels whose first draw lies in [first_draw, end_draw)
    const unsigned pix_lo = (first_draw + per_pixel - 1u) / per_pixel;
    const unsigned pix_hi = last_part ? npix : (end_draw + per_pixel - 1u) / per_pixel;
    const uint32_t* src = tile_rng + (static_cast<size_t>(tile) * p.stream_parts + part) * 624;
    for (int e = lane; e < 624; e += 64) st[e] = src[e];
    auto wave_sync = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    wave_sync();
    int cur = 0;
    unsigned pixels_done = pix_lo;
    for (unsigned done = first_draw; dst ? done < end_draw : pixels_done < pix_hi; done += 624u) {  // (a pixel's draws end before `total`)
        const uint32_t* o = st + cur * 624;
        uint32_t* n = st + (cur ^ 1) * 624;
        // mt19937 twist: new[k] from old[k], old[k+1] and old[k+397] (= new[k-227] once k >= 227); the
        // loops are unrolled so that a phase's LDS reads are all in flight before its first write
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = lane + 64 * i;
            if (k < 227) n[k] = mt_twist(o[k], o[k + 1], o[k + 397]);
        }
        wave_sync();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = 227 + lane + 64 * i;
            if (k < 454) n[k] = mt_twist(o[k], o[k + 1], n[k - 227]);
        }
        wave_sync();
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int k = 454 + lane + 64 * i;
            if (k < 624) n[k] = mt_twist(o[k], (k == 623) ? n[0] : o[k + 1], n[k - 227]);
        }
        wave_sync();
        cur ^= 1;
        const unsigned left = total - done;
        const int m = left < 624u ? static_cast<int>(left) : 624;
        if (dst && jitter_only) {  // wave-uniform; done is a multiple of 624 = 4 x 156: draw done + e is a jitter draw iff (e & 2) == 0
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int k = lane + 64 * i;  // the k-th jitter draw of this twist
                const int e = ((k >> 1) << 2) | (k & 1);
                if (e < m) dst[(done >> 1) + static_cast<unsigned>(k)] = mt_to_unit(mt_temper(n[e]));
            }
        } else if (dst) {
#pragma unroll
            for (int i = 0; i < 10; ++i) {
                const int e = lane + 64 * i;
                if (e < m) dst[done + e] = mt_to_unit(mt_temper(n[e]));
            }
        } else {
            // draws [done, done + m) are in n, the 624 before them in o (the previous twist's words).  Pixels
            // go in whole rounds of 64 (a twist completes only 624 / (2 spp) of them — 78 at 4 spp — and a
            // partial round costs as much as a full one); the rest waits for the next twist, except those
            // whose draws reach back into o, which that twist overwrites.
            const unsigned complete = min(pix_hi, (done + static_cast<unsigned>(m)) / per_pixel);
            const unsigned must_end = min(complete, (done + per_pixel - 1u) / per_pixel);  // first draw before `done`
            const unsigned pending = complete - pixels_done;
            unsigned take = (complete == pix_hi) ? pending : (pending / 64u) * 64u;
            if (pixels_done + take < must_end) take = must_end - pixels_done;
            if (take > 0u) {
                // (g and done are even: the pair is 8-byte aligned in either buffer — one LDS read instead of two, half the
                // cycles of the 8-lanes-per-bank stride a lane per pixel reads the stream with)
                background_pixels<kToPlate>(sc, p, tg, out_frame, out8, pixels_done, pixels_done + take, lane, [&](unsigned g, float& jx, float& jy) __attribute__((always_inline)) {
                    const uint2 w = *reinterpret_cast<const uint2*>((g >= done) ? n + (g - done) : o + (g + 624u - done));
                    jx = mt_to_unit(mt_temper(w.x));
                    jy = mt_to_unit(mt_temper(w.y));
                });
                pixels_done += take;
                wave_sync();  // the next twist overwrites o
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// queue helpers
// ---------------------------------------------------------------------------------------------
// counters[0]: number of planned units (one atomic add per touched tile, in plan_tiles)
constexpr int kCntDense = 8;              // general variants: counters[kCntDense + L] = entries of level L >= 1
constexpr int kCntDeep1 = kCntDense + 1;  // flat pipeline: level-1 records
// WaveSpace::end of a sample whose chain has ended: (records of the chain << 1) | stopped at maxBounces
constexpr uint32_t kEndMiss = 0xffffffffu;  // the primary ray missed: the sample's colour is the background at its jittered position
__device__ __forceinline__ uint32_t chain_code(int records, bool stopped_at_max) {
    return (static_cast<uint32_t>(records) << 1) | (stopped_at_max ? 1u : 0u);
}
constexpr int kCntUnits = 0;
constexpr int kCntTiles = 1;     // touched tiles of the batch so far
constexpr int kCntOverflow = kCounterWords - 1;  // set if more tiles are touched than the host planned for (a bug: the host
                                                 // bound is a superset); sticky

// The pass counters are never cleared: they run on from pass to pass (modulo 2^32), and what a pass has counted is the
// difference to `counter_base`, the snapshot `resolve` — the last kernel of every pass, in which nothing counts any more —
// takes for the pass that follows.  (A memset per pass was a dispatch of its own at the head of every frame: 3 us and a
// launch of a lone frame's 195.)  `resolve` itself reads the one count it needs from frame_info, which `primary` leaves.
__device__ __forceinline__ uint32_t counted(const WaveSpace& ws, int i) { return ws.counters[i] - ws.counter_base[i]; }
__device__ __forceinline__ uint32_t count_add(const WaveSpace& ws, int i, uint32_t n) { return atomicAdd(&ws.counters[i], n) - ws.counter_base[i]; }

// Work lists by ticket (`primary`, `lit`).  The items of these kernels' lists differ widely in cost — a unit without a hit
// is nothing, a full one a whole round, a chase block three dependent scene queries — and a grid smaller than the list
// (a frame that shares the device) that strides over it statically ends when its unluckiest workgroup does.  So a
// workgroup's FIRST item is blockIdx.x (no atomic, no burst at the kernel's start) and every later one is gridDim.x + a
// ticket: one more word of the pass counters per kernel, run on like the others (`resolve` snapshots it with them), each in
// a 128-byte line of its own (the level counters of the general variants end below word 4032).  Thread 0 claims; the item
// reaches the workgroup through LDS and one barrier (two slots taken in turn: a slot is written again only behind the
// barrier of the claim between, which every thread passes after reading it).  No workgroup ever waits for another: a
// ticket only grows, every claim is answered at once, and a workgroup leaves — all its threads, the item is uniform — with
// the first item at or past the end of the list, so the kernel ends after list + grid claims at the most.  A grid that
// covers the list takes no ticket at all.  p.work_tickets == 0: the static stride.  A ticket is, like every count, the
// word's difference to counter_base modulo 2^32: right across the word's wrap as long as a pass claims fewer than 2^32
// items, and gridDim.x + ticket stays below 2^32 for any list the 32-bit record indices allow.  (Claiming the NEXT ticket at
// the start of the current item, to hide the round trip, was measured and lost: DESIGN.md §4 "Measured and rejected: work
// tickets", profiles/work_tickets/README.md.)
constexpr int kCntTicketPrimary = kCounterWords - 64;
constexpr int kCntTicketLit = kCounterWords - 32;
__device__ __forceinline__ uint32_t next_work(const RenderParams& p, int word, uint32_t current, uint32_t end, uint32_t* s_ticket, uint32_t& turn) {
    if (!p.work_tickets || gridDim.x >= end) return current + gridDim.x;  // uniform
    uint32_t* slot = s_ticket + (turn++ & 1u);
    if (threadIdx.x == 0) *slot = gridDim.x + count_add(p.ws, word, 1u);
    __syncthreads();
    return *slot;
}

__device__ __forceinline__ void push_entry(const WaveSpace& ws, int parity, uint32_t e, const Ray& ray, const Hit& hit,
                                           uint32_t root, int depth) {
    ws.q_o[parity][e] = make_float4(ray.o.x, ray.o.y, ray.o.z, __uint_as_float(root));
    ws.q_d[parity][e] = make_float4(ray.d.x, ray.d.y, ray.d.z, __int_as_float(depth));
    ws.q_p[parity][e] = make_float4(hit.p.x, hit.p.y, hit.p.z, 0.0f);
    ws.q_n[parity][e] = make_float4(hit.n.x, hit.n.y, hit.n.z, 0.0f);
    ws.q_t[parity][e] = make_float4(hit.tex.r, hit.tex.g, hit.tex.b, hit.tex.a);
}

// ---- compact hit records of the flat pipeline (kernels.h: WaveSpace::q_*) -------------------------------
// .w of q_d: depth | face axis << 8 | min-side << 10 | exit-face << 11
__device__ __forceinline__ uint32_t record_code(int depth, const Hit& h) {
    return static_cast<uint32_t>(depth) | (static_cast<uint32_t>(h.axis) << 8) | (h.neg ? 1u << 10 : 0u) | (h.back ? 1u << 11 : 0u);
}
// with_origin: records below the primary hits, and primary hits under depth of field (otherwise the ray
// starts at the camera position)
__device__ __forceinline__ void push_record(const WaveSpace& ws, bool posed, uint32_t e, const Ray& ray, const Hit& hit, uint32_t root, int depth,
                                            bool with_origin) {
    ws.q_p[0][e] = make_float4(hit.p.x, hit.p.y, hit.p.z, __uint_as_float(root));
    ws.q_d[0][e] = make_float4(ray.d.x, ray.d.y, ray.d.z, __uint_as_float(record_code(depth, hit)));
    ws.q_x[e] = hit.texel;
    if (posed) ws.q_n[0][e] = make_float4(hit.n.x, hit.n.y, hit.n.z, 0.0f);
    if (with_origin) ws.q_o[0][e] = make_float4(ray.o.x, ray.o.y, ray.o.z, 0.0f);
}
// what the chain and shadow stages read of a record: hit point, normal (as intersectMesh returned it),
// ray direction, depth, root
struct RecordGeom {
    V3 p, n, d;
    uint32_t root;
    int depth;
};
__device__ __forceinline__ RecordGeom load_geom(const WaveSpace& ws, bool posed, uint32_t e) {
    const float4 qp = ws.q_p[0][e], qd = ws.q_d[0][e];
    const uint32_t code = __float_as_uint(qd.w);
    RecordGeom g;
    g.p = mk(qp.x, qp.y, qp.z);
    g.d = mk(qd.x, qd.y, qd.z);
    g.root = __float_as_uint(qp.w);
    g.depth = static_cast<int>(code & 0xffu);
    if (posed) {
        const float4 qn = ws.q_n[0][e];
        g.n = mk(qn.x, qn.y, qn.z);
    } else {
        g.n = unposed_normal(static_cast<int>((code >> 8) & 3u), ((code >> 10) & 1u) != 0u, ((code >> 11) & 1u) != 0u);
    }
    return g;
}
// only point and normal (a shadow or AO ray lane)
__device__ __forceinline__ void load_point_normal(const WaveSpace& ws, bool posed, uint32_t e, V3& P, V3& N) {
    const float4 qp = ws.q_p[0][e];
    P = mk(qp.x, qp.y, qp.z);
    if (posed) {
        const float4 qn = ws.q_n[0][e];
        N = mk(qn.x, qn.y, qn.z);
    } else {
        const uint32_t code = __float_as_uint(ws.q_d[0][e].w);
        N = unposed_normal(static_cast<int>((code >> 8) & 3u), ((code >> 10) & 1u) != 0u, ((code >> 11) & 1u) != 0u);
    }
}

// ---------------------------------------------------------------------------------------------
// plan_tiles: 1, 2 or 4 waves per tile of the batch — which meshes can touch the tile (tile_mesh_mask), its units and
// slot range (plan_touched_tile), then the tile's draws, a part of the stream per wave (tile_stream_wave)
// ---------------------------------------------------------------------------------------------
// which meshes' screen bounds touch the tile: lane m of the calling wave tests mesh m (pure: no side effects)
__device__ __forceinline__ unsigned long long tile_mesh_mask(const SceneView& sc, const RenderParams& p, const TileGeom& tg, int lane) {
    const mcrt_config& cfg = p.cfg;
    const bool dof = cfg.dof_enabled && cfg.aperture > 1e-6f;
    const bool cull = sc.hdr->cull_ok != 0 && sc.n_meshes < 64;
    const float aspect = static_cast<float>(cfg.width) / static_cast<float>(cfg.height);
    bool touch = lane < sc.n_meshes;
    if (touch && cull) {
        const FlatMesh& m = sc.meshes[lane];
        float lens_pad = 0.0f;
        if (dof) {
            // Thin lens (tile_renderer.cpp:42-69): the ray of screen sample s leaves the lens at offset
            // (lx, ly), |.| <= aperture, towards the focus point of the pinhole ray, so a point at
            // camera depth z on it is seen by the pinhole at s + (lx, ly) * (1/z - 1/zf), where
            // zf = focusDist / |(su, sv, 1)| is the depth of that focus point.  Over the mesh's depth
            // range and every zf of the frame this bounds the displacement; generous float slack.
            const float half_h = sc.hdr->cam_half_h, half_w = half_h * aspect;
            const float focus = cfg.focus_distance > 0.0f ? cfg.focus_distance : sc.hdr->cam_focus_auto;
            const float inv_f_lo = 1.0f / focus;
            const float inv_f_hi = __builtin_sqrtf(1.0f + half_w * half_w + half_h * half_h) / focus;
            const float inv_z_hi = 1.0f / m.depth[0], inv_z_lo = 1.0f / m.depth[1];
            const float d = fmaxf(fmaxf(fabsf(inv_z_hi - inv_f_lo), fabsf(inv_z_hi - inv_f_hi)),
                                  fmaxf(fabsf(inv_z_lo - inv_f_lo), fabsf(inv_z_lo - inv_f_hi)));
            lens_pad = cfg.aperture * d / half_h * 1.02f + 1e-3f;
            // That is the exact lens.  lens_ray forms the ray's origin (camera + lens offset) and its focus point (camera +
            // direction * focus) in floats at the camera's coordinate magnitude: each is off by up to an ulp of it, so the
            // direction, their difference of length ~ focus, is off by `err` / focus and the origin by `err`.  Far from the
            // origin (a camera 5e7 out: an ulp of 4 against a focus distance of 10) that is no small angle; from a twentieth
            // of the focus point's depth on there is no bound.  err: 4 ulp of the scene's magnitude (mask_slack / kMaskSlack).
            const float err = 4.0f * 1.1920929e-7f * (sc.hdr->mask_slack * (1.0f / kMaskSlack) + focus + cfg.aperture);
            const float r2 = half_w * half_w + half_h * half_h;
            const float rel = err * inv_f_hi * (1.0f + __builtin_sqrtf(r2));  // in tangent units, at the frame's corner
            lens_pad += (2.0f * rel + err * inv_z_hi) / half_h;
            if (!(m.depth[0] > 0.0f) || !(focus > 0.0f) || !(lens_pad < 1e6f) || !(rel < 0.05f)) lens_pad = 1e30f;  // no bound
        }
        touch = mesh_touches_tile(m, tg, cfg, aspect, lens_pad);
    }
    unsigned long long mask = __ballot(touch);
    if (!cull && sc.n_meshes > 0) mask = ~0ull;
    return mask;
}
// The units a touched tile is cut into (choose_parts_per_tile): their number, and unit i as a record (kernel_common.h) whose
// .x holds the form's flag alone and whose .w is the number of the tile's pixels in the units before it.  Pixel ranges: equal
// parts of the tile's row-major order.  Blocks: the grid's blocks that the (clipped) tile reaches, row by row, clipped with it.
__device__ __forceinline__ uint32_t tile_unit_count(const RenderParams& p, const TileGeom& tg) {
    if (p.unit_blocks)
        return static_cast<uint32_t>((tg.w + p.unit_bw - 1) / p.unit_bw) * static_cast<uint32_t>((tg.h + p.unit_bh - 1) / p.unit_bh);
    const uint32_t npix = static_cast<uint32_t>(tg.w) * static_cast<uint32_t>(tg.h);  // npix * spp <= ws.tile_slots
    const uint32_t parts = static_cast<uint32_t>(p.parts_per_tile);
    const uint32_t per = (npix + parts - 1u) / parts;
    return (npix + per - 1u) / per;
}
__device__ __forceinline__ uint4 tile_unit(const RenderParams& p, const TileGeom& tg, uint32_t i) {
    if (p.unit_blocks) {
        const uint32_t cols = static_cast<uint32_t>((tg.w + p.unit_bw - 1) / p.unit_bw);
        const uint32_t by = i / cols, bx = i - by * cols;
        const uint32_t x0 = bx * static_cast<uint32_t>(p.unit_bw), y0 = by * static_cast<uint32_t>(p.unit_bh);
        const uint32_t w = min(static_cast<uint32_t>(p.unit_bw), static_cast<uint32_t>(tg.w) - x0);
        const uint32_t h = min(static_cast<uint32_t>(p.unit_bh), static_cast<uint32_t>(tg.h) - y0);
        return make_uint4(kUnitBlock, x0 | (y0 << 16), w | (h << 16), y0 * static_cast<uint32_t>(tg.w) + h * x0);
    }
    const uint32_t npix = static_cast<uint32_t>(tg.w) * static_cast<uint32_t>(tg.h);
    const uint32_t parts = static_cast<uint32_t>(p.parts_per_tile);
    const uint32_t per = (npix + parts - 1u) / parts;
    const uint32_t a = i * per;
    return make_uint4(0u, a, min(npix, a + per), a);
}
// The tile's wave: units and slot range of a tile that meshes can touch; returns its number among the batch's touched tiles
// (the same in every lane), ~0u for a tile that is not queued.  A lane per unit writes the records.
__device__ __forceinline__ uint32_t plan_touched_tile(const RenderParams& p, const TileGeom& tg, int tile, unsigned long long mask, int lane) {
    const mcrt_config& cfg = p.cfg;
    const WaveSpace& ws = p.ws;
    if (lane == 0) ws.tile_mask[tile] = mask;
    if (mask == 0ull) return ~0u;  // background tile: never queued
    const uint32_t spp = cfg.samples_per_pixel > 1 ? cfg.samples_per_pixel : 1;
    const uint32_t used = tile_unit_count(p, tg);
    // the k-th touched tile of the batch owns slot range k: the workspace is sized for the tiles that can
    // be touched (host-side superset), not for every sample of the batch
    uint32_t ord = 0, slot0 = 0;
    if (lane == 0) {
        ord = count_add(ws, kCntTiles, 1u);
        if (ord >= ws.tile_cap) {  // cannot happen; keep memory safe and leave a mark if it ever does
            ws.counters[kCntOverflow] = 1u;
            ws.tile_mask[tile] = 0ull;
            ord = ~0u;
        } else {
            slot0 = count_add(ws, kCntUnits, used);
        }
    }
    ord = static_cast<uint32_t>(__shfl(static_cast<int>(ord), 0));
    slot0 = static_cast<uint32_t>(__shfl(static_cast<int>(slot0), 0));
    if (ord == ~0u) return ~0u;
    const uint32_t base = ord * ws.tile_slots;
    for (uint32_t i = static_cast<uint32_t>(lane); i < used; i += 64u) {
        const uint4 u = tile_unit(p, tg, i);
        ws.units[slot0 + i] = make_uint4(static_cast<uint32_t>(tile) | u.x, u.y, u.z, base + u.w * spp);
    }
    return ord;
}

__device__ __forceinline__ void plan_tiles_body(const uint8_t* __restrict__ scene_blob, const uint32_t* __restrict__ tile_rng,
                                                float* __restrict__ tile_draws, float4* __restrict__ out_frame, uchar4* __restrict__ out8,
                                                const RenderParams& __restrict__ p, const int tile_base, const int n_tiles) {
    __shared__ __align__(16) uint32_t s_state[kStreamWaves][2 * 624];
    __shared__ uint32_t s_ord[kStreamWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // `parts` neighbouring waves of the workgroup share a tile (1, 2 or 4: a power of two that divides kStreamWaves), each
    // taking `per_wave` consecutive parts of the tile's stream
    const int parts = p.stream_waves;
    const int per_wave = p.stream_parts / parts;
    const int slot = static_cast<int>(blockIdx.x) * kStreamWaves + wave;
    const int t = slot / parts, part = slot - t * parts;
    const bool valid = t < n_tiles;  // wave-uniform
    const int tile = tile_base + (valid ? t : 0);
    const TileGeom tg = tile_of(p, tile);
    const SceneView sc = view_of(scene_blob);
    // the tile's mesh mask: every wave of the tile forms it (the same ballot); its slot range and units: the first wave
    const unsigned long long mask = valid ? tile_mesh_mask(sc, p, tg, lane) : 0ull;
    if (valid && part == 0) {  // wave-uniform
        const uint32_t planned = plan_touched_tile(p, tg, tile, mask, lane);
        if (lane == 0) s_ord[wave] = planned;
    }
    if (parts > 1) {
        __syncthreads();  // the only workgroup barrier of the kernel: the tile's number among the touched tiles
    } else {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (!valid) return;
    const uint32_t ord = s_ord[wave - part];
    const size_t stride = p.ws.draws_stride;
    const unsigned npix = static_cast<unsigned>(tg.w) * static_cast<unsigned>(tg.h);
    if (!p.bg_in_plan) {  // every tile's draws to HBM; `primary` renders the background tiles (those of one colour need no draws)
        float4 unused;
        if (p.draws_per_sample > 0 && !(mask == 0ull && constant_background(sc, p, tg, unused)))
            tile_stream_wave(sc, tile_rng, tile_draws + static_cast<size_t>(t) * stride, nullptr, nullptr, p, tg, tile, part * per_wave, per_wave, s_state[wave], lane,
                             /*jitter_only=*/mask == 0ull && p.draws_per_sample == 4);
    } else if (mask != 0ull) {  // a tile meshes can touch: its draws, at its touched-tile number — unless the device's draw plate holds them
        if (p.draws_per_sample > 0 && ord != ~0u && !p.draw_plate)
            tile_stream_wave(sc, tile_rng, tile_draws + static_cast<size_t>(ord) * stride, nullptr, nullptr, p, tg, tile, part * per_wave, per_wave, s_state[wave], lane);
    } else if (p.background == MCRT_BACKGROUND_TRANSPARENT) {  // no sample of the tile can hit: (0,0,0,0), no draws (bg_in_plan is 1)
        fill_tile(p, tg, out_frame, out8, make_float4(0.0f, 0.0f, 0.0f, 0.0f), static_cast<unsigned>(part * 64 + lane), static_cast<unsigned>(parts) * 64u);
    } else if (float4 pixel; constant_background(sc, p, tg, pixel)) {  // background tile of one colour: no draws, no samples
        fill_tile(p, tg, out_frame, out8, pixel, static_cast<unsigned>(part * 64 + lane), static_cast<unsigned>(parts) * 64u);
    } else if (p.cfg.samples_per_pixel > 1) {  // background tile, jittered samples: from the device's plate when the frame has one
        if (p.bg_plate)
            copy_plate_tile(p, tg, out_frame, out8, static_cast<unsigned>(part * 64 + lane), static_cast<unsigned>(parts) * 64u);
        else
            tile_stream_wave(sc, tile_rng, nullptr, out_frame, out8, p, tg, tile, part * per_wave, per_wave, s_state[wave], lane);
    } else {  // background tile, one centred sample per pixel: no draws at all
        background_pixels(sc, p, tg, out_frame, out8, npix * static_cast<unsigned>(part) / static_cast<unsigned>(parts),
                          npix * static_cast<unsigned>(part + 1) / static_cast<unsigned>(parts), lane,
                          [](unsigned, float&, float&) __attribute__((always_inline)) {});
    }
}
__global__ __launch_bounds__(64 * kStreamWaves) void plan_tiles_kernel(const uint8_t* __restrict__ scene_blob,
                                                                       const uint32_t* __restrict__ tile_rng,
                                                                       float* __restrict__ tile_draws, float4* __restrict__ out_frame,
                                                                       uchar4* __restrict__ out8, const RenderParams p,
                                                                       const int tile_base, const int n_tiles) {
    plan_tiles_body(scene_blob, tile_rng, tile_draws, out_frame, out8, p, tile_base, n_tiles);
}

// Fills a background plate (kernels.h): every tile of the frame that is not of one colour, by `plan_tiles`' own routine for
// a gradient background tile — whether or not meshes touch the tile in some scene.  p: a whole-frame shard, one wave per
// stream part; p.scene is not read beyond its header (gradient background).
__global__ __launch_bounds__(64 * kStreamWaves) void fill_bg_plate_kernel(const RenderParams p, float4* __restrict__ plate, const int n_tiles) {
    __shared__ __align__(16) uint32_t s_state[kStreamWaves][2 * 624];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int parts = p.stream_parts;  // 1, 2 or 4: divides kStreamWaves
    const int slot = static_cast<int>(blockIdx.x) * kStreamWaves + wave;
    const int tile = slot / parts, part = slot - tile * parts;
    if (tile >= n_tiles) return;  // wave-uniform; no workgroup barrier in this kernel
    const TileGeom tg = tile_of(p, tile);
    const SceneView sc = view_of(p.scene);
    float4 unused;
    if (constant_background(sc, p, tg, unused)) return;
    tile_stream_wave<true>(sc, p.tile_rng, nullptr, plate, nullptr, p, tg, tile, part, 1, s_state[wave], lane);
}

// Fills a draw plate (kernels.h): the draws of every tile of the frame, by `plan_tiles`' own routine for a touched tile, into
// the tile's slot of the plate.  p: a whole-frame shard, one wave per stream part; p.scene is not read beyond its header.
__global__ __launch_bounds__(64 * kStreamWaves) void fill_draw_plate_kernel(const RenderParams p, float* __restrict__ plate, const int n_tiles) {
    __shared__ __align__(16) uint32_t s_state[kStreamWaves][2 * 624];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int parts = p.stream_parts;  // 1, 2 or 4: divides kStreamWaves
    const int slot = static_cast<int>(blockIdx.x) * kStreamWaves + wave;
    const int tile = slot / parts, part = slot - tile * parts;
    if (tile >= n_tiles) return;  // wave-uniform; no workgroup barrier in this kernel
    const TileGeom tg = tile_of(p, tile);
    const SceneView sc = view_of(p.scene);  // (a stream with a destination renders nothing: the view is not used)
    tile_stream_wave(sc, p.tile_rng, plate + static_cast<size_t>(tg.frame_tile) * p.ws.draws_stride, nullptr, nullptr, p, tg, tile, part, 1, s_state[wave], lane);
}

// The engine states at the starts of a tile's parts 1 .. parts-1 (tile_stream_wave): one wave per tile twists the seeded
// state part_twists times per part, in LDS, and stores where it stands.  A function of the seeds and of part_twists only:
// run with the tile seeds, kept across renders with them.
__device__ __forceinline__ void advance_tiles_body(const RenderParams& __restrict__ p, int n_tiles) {
    __shared__ __align__(16) uint32_t s_state[kStreamWaves][2 * 624];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = static_cast<int>(blockIdx.x) * kStreamWaves + wave;
    if (tile >= n_tiles) return;  // wave-uniform; no workgroup barrier in this kernel
    uint32_t* st = s_state[wave];
    uint32_t* states = p.tile_rng + static_cast<size_t>(tile) * p.stream_parts * 624;
    for (int e = lane; e < 624; e += 64) st[e] = states[e];
    auto wave_sync = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    wave_sync();
    int cur = 0;
    for (int part = 1; part < p.stream_parts; ++part) {
        for (int k = 0; k < p.stream_part_twists; ++k) {
            const uint32_t* o = st + cur * 624;
            uint32_t* n = st + (cur ^ 1) * 624;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = lane + 64 * i;
                if (e < 227) n[e] = mt_twist(o[e], o[e + 1], o[e + 397]);
            }
            wave_sync();
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = 227 + lane + 64 * i;
                if (e < 454) n[e] = mt_twist(o[e], o[e + 1], n[e - 227]);
            }
            wave_sync();
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int e = 454 + lane + 64 * i;
                if (e < 624) n[e] = mt_twist(o[e], (e == 623) ? n[0] : o[e + 1], n[e - 227]);
            }
            wave_sync();
            cur ^= 1;
        }
        const uint32_t* now = st + cur * 624;
        for (int e = lane; e < 624; e += 64) states[static_cast<size_t>(part) * 624 + e] = now[e];
    }
}
__global__ __launch_bounds__(64 * kStreamWaves) void advance_tiles_kernel(RenderParams p, int n_tiles) { advance_tiles_body(p, n_tiles); }

// ---------------------------------------------------------------------------------------------
// primary: persistent workgroups; touched units first, then the background tiles.  A sample's draws
// sit in tile_draws at ((pixel in tile) * spp + sample) * draws_per_sample.
// ---------------------------------------------------------------------------------------------
// 5 waves per SIMD (96 VGPRs, four of them spilled) instead of the 4 the unconstrained build settles at (105 VGPRs): same-box
// A/B +1.5 % at four frames in flight and, with 1280 workgroups, -8 us for one frame alone (profiles/r03_experiments)
#ifndef MCRT_PRIMARY_WAVES
#define MCRT_PRIMARY_WAVES 5
#endif
template <int kView>
__device__ __forceinline__ void primary_body(const uint8_t* __restrict__ scene_blob, const float* __restrict__ tile_draws,
                                             float4* __restrict__ out_frame, uchar4* __restrict__ out8, const ParamPtr pp,
                                             const int tile_base, const int n_tiles) {
    __shared__ int s_wcnt[kBlock / 64];
    __shared__ float4 s_bd[kBlock], s_bp[kBlock], s_bn[kBlock];  // the chunk's primary hits, packed, for their reflection rays
    __shared__ uint32_t s_out_base;
    __shared__ uint32_t s_ticket[2];
    extern __shared__ __align__(16) unsigned char s_dyn[];

    // The parameters by phase (kernel_common.h, phase_params): across the unit loop live the loop's own state, the scene
    // view and `pp` — every phase below reads what it needs of the parameters where it begins.
    const SceneView scg = view_of(scene_blob);
    const int tid = threadIdx.x;
    uint32_t n_units;
    {  // ---- entry: the pass's unit count, and whether this workgroup has anything to do
        const RenderParams& p = phase_params(pp);
        n_units = counted(p.ws, kCntUnits);
        if (blockIdx.x == 0 && threadIdx.x == 0) p.ws.frame_info[0] = n_units;  // for `resolve`, which takes the next pass's counter base
        if ((p.bg_in_plan || p.bg_kernel) && blockIdx.x >= n_units) return;  // nothing for this workgroup: leave before the collective staging
    }
    const typename ViewSel<kView>::type sc = ViewSel<kView>::make(scg, phase_params(pp), s_dyn);

    // ================= units of tiles that meshes can touch: thread per sample =================
    // (the list by ticket: next_work)
    uint32_t turn = 0;
    for (uint32_t u = blockIdx.x; u < n_units; u = next_work(phase_params(pp), kCntTicketPrimary, u, n_units, s_ticket, turn)) {
        // ---- phase: the unit — its record, its tile, where its draws are
        const RenderParams& pu = phase_params(pp);
        const uint4 ud = pu.ws.units[u];
        const int tile = unit_tile(ud);
        const uint32_t slot_base = ud.w;
        const int spp_u = pu.cfg.samples_per_pixel > 1 ? pu.cfg.samples_per_pixel : 1;
        const unsigned n_samples = unit_pixels(ud) * static_cast<unsigned>(spp_u);
        const TileGeom tg = tile_of(pu, tile);
        const unsigned long long mesh_mask = pu.ws.tile_mask[tile];
        // the tile's draws: in the draw plate (tile_draws is then the plate) at its index in the frame; else at its touched-tile
        // number, or (all tiles' streams in HBM) at its index in the batch
        const float* draws = tile_draws + static_cast<size_t>(pu.draw_plate ? static_cast<uint32_t>(tg.frame_tile)
                                                              : pu.bg_in_plan ? slot_base / pu.ws.tile_slots : static_cast<uint32_t>(tile - tile_base)) *
                                              static_cast<size_t>(pu.ws.draws_stride);
        // the unit's pixels (kernel_common.h); its origin folded into the frame position and the draws' address, which leaves the
        // loop below the column and row inside the unit's rectangle
        const UnitMap um(ud, tg);
        const int px0 = tg.x + static_cast<int>(um.x0), py0 = tg.y + static_cast<int>(um.y0);
        const unsigned tile_w = static_cast<unsigned>(tg.w);
        const float* unit_draws = draws + static_cast<size_t>(um.y0 * tile_w + um.x0) * spp_u * pu.draws_per_sample;

        uint32_t unit_hits = 0;  // hits so far: they occupy slots slot_base .. slot_base + unit_hits
        for (unsigned s0 = 0; s0 < n_samples; s0 += kChunk) {  // uniform trip count
            bool is_hit = false;
            Ray ray{mk(0, 0, 0), mk(0, 0, 0)};
            Hit hit;
            hit.hit = false;
            uint32_t sample_slot = 0;
            const unsigned sidx = s0 + tid;  // sample of the unit, in stream order
            if (sidx < n_samples) {
                // ---- phase: the camera ray of the sample and its closest hit
                const RenderParams& p = phase_params(pp);
                const mcrt_config& cfg = p.cfg;
                const int spp = cfg.samples_per_pixel > 1 ? cfg.samples_per_pixel : 1;
                const int dd = p.draws_per_sample;
                const bool dof = cfg.dof_enabled && cfg.aperture > 1e-6f;
                const float aspect = static_cast<float>(cfg.width) / static_cast<float>(cfg.height);
                const FrameDiv fd(p);
                const unsigned k = UDiv(static_cast<unsigned>(spp)).div(sidx);  // pixel of the unit; sidx - k * spp: its sample
                unsigned col, row;
                um.rel(k, col, row);
                const int px = px0 + static_cast<int>(col), py = py0 + static_cast<int>(row);
                const float* jd = unit_draws + (static_cast<size_t>(row * tile_w + col - k) * spp + sidx) * dd;  // ((ly w + lx) spp + s) dd, s = sidx - k spp
                float jx = 0.5f, jy = 0.5f;
                int dpos = 0;
                if (spp > 1) {
                    jx = jd[0];
                    jy = jd[1];
                    dpos = 2;
                }
                const float su = fd.u(static_cast<float>(px) + jx);
                const float sv = fd.v(static_cast<float>(py) + jy);
                sample_slot = slot_base + sidx;
                if (dof) {
                    float focusDist = cfg.focus_distance;
                    if (focusDist <= 0.0f) focusDist = sc.hdr->cam_focus_auto;
                    ray = lens_ray(sc, su, sv, aspect, cfg.aperture, focusDist, jd[dpos], jd[dpos + 1]);
                } else {
                    ray = camera_ray(sc, su, sv, aspect);
                }
                hit = hit_scene(sc, ray, mesh_mask);
            }
            // ---- phase: how the sample ends, and the hits' records
            const RenderParams& q = phase_params(pp);
            const bool flat = q.flat != 0;
            const bool bounce_here = flat && q.cfg.max_bounces >= 1;
            if (sidx < n_samples) {
                // A miss: its colour is a function of the sample's jitter pair alone (tile_renderer.cpp:111-114) — `resolve`
                // forms it from the pair in the tile's stream (8 B) instead of a colour stored here and read back there
                // (2 x 16 B per miss of a touched tile: 13 MB of the metric frame's counted HBM traffic).
                uint32_t code = kEndMiss;
                if (hit.hit && q.cfg.max_bounces < 0) {
                    const C4 col = background(sc, q.cfg, 0.5f, 0.5f);  // raytracer.cpp:86-90 (depth 0 > maxBounces)
                    q.ws.scol[sample_slot] = make_float4(col.r, col.g, col.b, col.a);
                    code = 0u;
                } else if (hit.hit) {
                    is_hit = true;
                    // 0: the colour is in scol (general variants: `level_shade` puts the hits' colours there).  Flat pipeline:
                    // the second phase below / `lit` overwrite a hit's word with its chain's end code — unless maxBounces is 0
                    // and the chain is its primary hit alone.
                    code = (flat && q.cfg.max_bounces == 0) ? 3u : 0u;
                }
                q.ws.end[sample_slot] = code;
            }
            // hits → dense entries at the front of the unit's slot range (no global atomics)
            int total = 0;
            const int rank = block_rank(is_hit, s_wcnt, total);
            if (is_hit) {
                const uint32_t e = slot_base + unit_hits + static_cast<uint32_t>(rank);
                // root of the chain = its sample's colour slot
                if (flat)
                    push_record(q.ws, kView != kViewLdsUnposed && q.scene_posed != 0, e, ray, hit, sample_slot, 0, q.cfg.dof_enabled && q.cfg.aperture > 1e-6f);
                else
                    push_entry(q.ws, 0, e, ray, hit, sample_slot, 0);
                if (bounce_here) {
                    s_bd[rank] = make_float4(ray.d.x, ray.d.y, ray.d.z, __uint_as_float(sample_slot));
                    s_bp[rank] = make_float4(hit.p.x, hit.p.y, hit.p.z, 0.0f);
                    s_bn[rank] = make_float4(hit.n.x, hit.n.y, hit.n.z, 0.0f);
                }
            }
            unit_hits += static_cast<uint32_t>(total);
            // flat pipeline: the reflection ray of every primary hit (raytracer.cpp:133-139) is traced right here, by the first
            // `total` threads of the block on the chunk's packed hits (as a launch of its own this stage re-read every record:
            // 39 + 28 us became 59 us)
            if (bounce_here && total > 0) {  // uniform
                __syncthreads();
                bool next_hit = false;
                Ray nray{mk(0, 0, 0), mk(0, 0, 0)};
                Hit nhit;
                nhit.hit = false;
                uint32_t root = 0;
                if (tid < total) {
                    const float4 bd = s_bd[tid], bp = s_bp[tid], bn = s_bn[tid];
                    root = __float_as_uint(bd.w);
                    nray = reflect_ray(mk(bd.x, bd.y, bd.z), mk(bp.x, bp.y, bp.z), mk(bn.x, bn.y, bn.z));
                    nhit = hit_scene<true>(sc, nray, ~0ull);
                }
                // ---- phase: the level-1 records
                const RenderParams& r = phase_params(pp);
                if (tid < total) {
                    if (nhit.hit)
                        next_hit = true;
                    else
                        r.ws.end[root] = chain_code(1, false);  // bounced ray missed → flat background (raytracer.cpp:94-102)
                }
                int survivors = 0;
                const int srank = block_rank(next_hit, s_wcnt, survivors);
                if (survivors > 0) {  // uniform
                    if (tid == 0) s_out_base = count_add(r.ws, kCntDeep1, static_cast<uint32_t>(survivors));
                    __syncthreads();
                    if (next_hit)
                        push_record(r.ws, kView != kViewLdsUnposed && r.scene_posed != 0, r.ws.cap + s_out_base + static_cast<uint32_t>(srank), nray, nhit, root, 1, true);
                }
                __syncthreads();  // s_bd .. s_out_base are reused by the next chunk
            }
        }
        if (tid == 0) phase_params(pp).ws.unit_hits[u] = unit_hits;
    }


    // ================= background tiles: nothing can be hit, no ray is needed =================
    // (only when a pixel takes more than 24 draws — otherwise `plan_tiles` has rendered them from LDS — and at most
    // kSlabMinSpp - 1 samples: above that `background_kernel` does it)
    // thread per pixel, its samples in order as renderTile sums them (tile_renderer.cpp:116-124); no barriers
    const RenderParams& p = phase_params(pp);
    if (p.bg_in_plan || p.bg_kernel) return;
    const mcrt_config& cfg = p.cfg;
    const WaveSpace& ws = p.ws;
    const int spp = cfg.samples_per_pixel > 1 ? cfg.samples_per_pixel : 1;
    const FrameDiv fd(p);
    const size_t stride = ws.draws_stride;
    const float inv_spp = 1.0f / static_cast<float>(spp);
    for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int tile = tile_base + t;
        if (ws.tile_mask[tile] != 0ull) continue;  // uniform
        const TileGeom tg = tile_of(p, tile);
        if (float4 pixel; constant_background(scg, p, tg, pixel)) {  // uniform
            fill_tile(p, tg, out_frame, out8, pixel, static_cast<unsigned>(tid), static_cast<unsigned>(kBlock));
            continue;
        }
        const unsigned npix = static_cast<unsigned>(tg.w) * static_cast<unsigned>(tg.h);
        // the tile's jitter pairs, pixel-major (under depth of field a background tile's stream holds them only, packed: tile_stream_wave)
        const float2* pairs = reinterpret_cast<const float2*>(tile_draws + static_cast<size_t>(t) * stride);
        for (unsigned pix = tid; pix < npix; pix += kBlock) {
            const unsigned uly = pix / static_cast<unsigned>(tg.w);
            const int ly = static_cast<int>(uly);
            const int lx = static_cast<int>(pix - uly * static_cast<unsigned>(tg.w));
            const float fx = static_cast<float>(tg.x + lx), fy = static_cast<float>(tg.y + ly);
            const float2* jd = pairs + static_cast<size_t>(pix) * spp;
            float ar = 0.0f, ag = 0.0f, ab = 0.0f, aa = 0.0f;
            for (int sidx = 0; sidx < spp; ++sidx) {
                const float2 j = jd[sidx];
                const C4 c = background(sc, cfg, fd.u(fx + j.x), fd.v(fy + j.y));  // tile_renderer.cpp:111-114
                ar += c.r;
                ag += c.g;
                ab += c.b;
                aa += c.a;
            }
            const int row = (p.layout == MCRT_LAYOUT_PACKED) ? ((p.shard.pack_first + tg.owned_row * p.shard.pack_step) * cfg.tile_size + ly) : (tg.y + ly);
            store_pixel(out_frame, out8, static_cast<size_t>(row) * cfg.width + (tg.x + lx),
                        make_float4(ar * inv_spp, ag * inv_spp, ab * inv_spp, aa * inv_spp));
        }
    }
}
template <int kView>
__global__ __launch_bounds__(kBlock, MCRT_PRIMARY_WAVES) void primary_kernel(const RenderParams p, const uint8_t* __restrict__ scene_blob,
                                                         const float* __restrict__ tile_draws,
                                                         float4* __restrict__ out_frame, uchar4* __restrict__ out8,
                                                         const int tile_base, const int n_tiles) {
    primary_body<kView>(scene_blob, tile_draws, out_frame, out8, kernarg_params(), tile_base, n_tiles);
}

// ---------------------------------------------------------------------------------------------
// background: the tiles no mesh can touch at HIGH sample counts (kSlabMinSpp samples per pixel and more; below that the
// loop above, in `primary`'s tail, does as well).  The tile's stream in HBM is pixel-major — a pixel's spp jitter pairs
// side by side, 8·spp bytes per pixel — so a lane per pixel reads it at a stride of 8·spp bytes: at 64 spp that is 64 cache
// lines per load instruction and 32 KB of lines per wave in flight, more than the L1 holds: the loop was bound by those
// transactions (8.4 of the 8K / 64 spp frame's 14.3 ms per pass).  Here a wave fetches a SLAB — 64 pixels x 16 samples — with
// neighbouring lanes on neighbouring pairs (every line touched once and used whole), parks it in LDS with the pixels' rows
// padded by one pair (a lane per pixel then reads at a stride of 34 words: two lanes per bank) and consumes it, a lane per
// pixel, samples in order (tile_renderer.cpp:116-124); waves work on their own: no workgroup barrier.  8K / 64 spp: 20.4 ->
// 17.1 ms alone; at 16 spp the staging costs 3-5 % more than it saves (same-box A/B, profiles/r03_experiments).
// ---------------------------------------------------------------------------------------------
constexpr int kSlabSamples = 16;
#ifndef MCRT_BG_WAVES
#define MCRT_BG_WAVES 3
#endif
__device__ __forceinline__ void background_body(const uint8_t* __restrict__ scene_blob, const float* __restrict__ tile_draws,
                                                float4* __restrict__ out_frame, uchar4* __restrict__ out8, const RenderParams& __restrict__ p,
                                                const int tile_base, const int n_tiles) {
    __shared__ __align__(16) float2 s_slab[kBlock / 64][64][kSlabSamples + 1];
    const SceneView sc = view_of(scene_blob);
    const mcrt_config& cfg = p.cfg;
    const WaveSpace& ws = p.ws;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned spp = static_cast<unsigned>(cfg.samples_per_pixel > 1 ? cfg.samples_per_pixel : 1);
    const FrameDiv fd(p);
    const float inv_spp = 1.0f / static_cast<float>(spp);
    const size_t stride = ws.draws_stride;
    float2(*slab)[kSlabSamples + 1] = s_slab[wave];
    auto wave_sync = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int tile = tile_base + t;
        if (ws.tile_mask[tile] != 0ull) continue;  // uniform
        const TileGeom tg = tile_of(p, tile);
        if (float4 pixel; constant_background(sc, p, tg, pixel)) {  // uniform
            fill_tile(p, tg, out_frame, out8, pixel, threadIdx.x, static_cast<unsigned>(kBlock));
            continue;
        }
        const unsigned npix = static_cast<unsigned>(tg.w) * static_cast<unsigned>(tg.h);
        // the tile's jitter pairs, pixel-major: pair s of pixel q at pairs[q * spp + s] (under depth of field the stream of a
        // background tile holds the jitter pairs only, packed: tile_stream_wave)
        const float2* pairs = reinterpret_cast<const float2*>(tile_draws + static_cast<size_t>(t) * stride);
        const UDiv by_w(static_cast<unsigned>(tg.w));
        for (unsigned g0 = static_cast<unsigned>(wave) * 64u; g0 < npix; g0 += kBlock) {  // this wave's groups of 64 pixels
            const unsigned group = min(64u, npix - g0);
            const unsigned pix = g0 + static_cast<unsigned>(lane);
            const unsigned uly = by_w.div(pix);
            const int ly = static_cast<int>(uly);
            const int lx = static_cast<int>(pix - uly * static_cast<unsigned>(tg.w));
            const float fx = static_cast<float>(tg.x + lx), fy = static_cast<float>(tg.y + ly);
            float ar = 0.0f, ag = 0.0f, ab = 0.0f, aa = 0.0f;
            // A full slab (64 pixels x 16 samples) is fetched into registers one slab AHEAD: lane l takes pair l % 16 of
            // pixels l / 16, l / 16 + 4, ... — 16 loads, a pixel's 128 bytes across 16 lanes — issued before the previous
            // slab is consumed, parked in LDS after it: the loads' latency runs under 1 024 background samples.
            float2 ahead[kSlabSamples];
            const float2* mine = pairs + static_cast<size_t>(g0 + (static_cast<unsigned>(lane) >> 4)) * spp + (static_cast<unsigned>(lane) & 15u);
            auto fetch_ahead = [&](unsigned s0) __attribute__((always_inline)) {
#pragma unroll
                for (int i = 0; i < kSlabSamples; ++i) ahead[i] = mine[static_cast<size_t>(4 * i) * spp + s0];
            };
            const bool full_group = group == 64u;
            if (full_group && spp >= static_cast<unsigned>(kSlabSamples)) fetch_ahead(0u);
            for (unsigned s0 = 0; s0 < spp; s0 += kSlabSamples) {  // uniform
                const unsigned ns = min(static_cast<unsigned>(kSlabSamples), spp - s0);
                if (full_group && ns == static_cast<unsigned>(kSlabSamples)) {  // uniform
#pragma unroll
                    for (int i = 0; i < kSlabSamples; ++i) slab[4 * i + (lane >> 4)][lane & 15] = ahead[i];
                    if (s0 + 2u * kSlabSamples <= spp) fetch_ahead(s0 + kSlabSamples);  // the next slab is a full one too
                } else {
                    const UDiv by_ns(ns);
                    const unsigned items = group * ns;
                    for (unsigned c = static_cast<unsigned>(lane); c < items; c += 64u) {  // neighbouring lanes, neighbouring pairs
                        const unsigned q = by_ns.div(c), k = c - q * ns;
                        slab[q][k] = pairs[static_cast<size_t>(g0 + q) * spp + s0 + k];
                    }
                }
                wave_sync();
                if (static_cast<unsigned>(lane) < group) {
                    for (unsigned k = 0; k < ns; ++k) {
                        const float2 j = slab[lane][k];
                        const C4 col = background(sc, cfg, fd.u(fx + j.x), fd.v(fy + j.y));  // tile_renderer.cpp:111-114
                        ar += col.r;
                        ag += col.g;
                        ab += col.b;
                        aa += col.a;
                    }
                }
                wave_sync();  // the next slab overwrites this one
            }
            if (static_cast<unsigned>(lane) < group) {
                const int row = (p.layout == MCRT_LAYOUT_PACKED) ? ((p.shard.pack_first + tg.owned_row * p.shard.pack_step) * cfg.tile_size + ly) : (tg.y + ly);
                store_pixel(out_frame, out8, static_cast<size_t>(row) * cfg.width + (tg.x + lx), make_float4(ar * inv_spp, ag * inv_spp, ab * inv_spp, aa * inv_spp));
            }
        }
    }
}
__global__ __launch_bounds__(kBlock, MCRT_BG_WAVES) void background_kernel(const uint8_t* __restrict__ scene_blob, const float* __restrict__ tile_draws,
                                                            float4* __restrict__ out_frame, uchar4* __restrict__ out8, const RenderParams p,
                                                            const int tile_base, const int n_tiles) {
    background_body(scene_blob, tile_draws, out_frame, out8, p, tile_base, n_tiles);
}

// ---------------------------------------------------------------------------------------------
// The recursion of RayTracer::traceRay (raytracer.cpp:82-148) as a FLAT pipeline.  The reflection ray
// of a hit depends on geometry only — direction, hit point, normal (:133-139) — not on the colour
// of the hit.  So the chain of hits below a primary hit is chased first (`primary`'s second phase: every
// primary hit's reflection ray; the head of `lit`: the ~10 % that hit again, followed to their end), every hit of every
// level becoming one *record*; then the expensive stages — light samples, shadow rays, shading — run ONCE over
// all records of all levels, and `resolve` folds each chain's level colours back to front (:143-147)
// while it sums the pixel's samples.  One launch set per level cost ~40 us of dependent latency per
// level whatever it held (320 k, 31 k, 3 k, 300, 30 records at 1080p / 4 spp).
//
// Primary hits sit at the front of each unit's slot range (count per unit, no atomics).  Level-1 records are
// appended densely behind index `cap` by `primary` with ONE workgroup-aggregated atomic per 256-entry block (counter
// kCntDeep1); the records of levels >= 2 go to per-block regions behind them and never meet a global counter (`lit`).
// The general variants (per-hit RNG streams longer than the register engine, or more bounces than
// the flat record arrays are laid out for) keep one launch set per level with ping-pong queues.
// ---------------------------------------------------------------------------------------------

// which records a queue kernel walks: flat — every record of the batch; else — the entries of `level`
struct Scope {
    int level;
    int flat;
    __device__ __forceinline__ bool units() const { return flat || level == 0; }  // records at the front of the units' slot ranges
    __device__ __forceinline__ bool dense() const { return flat || level > 0; }   // records in the dense queue
    __device__ __forceinline__ int par() const { return flat ? 0 : (level & 1); }
};
__device__ __forceinline__ uint32_t dense_count(const WaveSpace& ws, Scope s) {
    return s.flat ? counted(ws, kCntDeep1) : counted(ws, kCntDense + s.level);  // (flat: the level-1 records; deeper ones are private to `lit`'s chasing blocks)
}
__device__ __forceinline__ uint32_t dense_base(const WaveSpace& ws, Scope s) { return s.flat ? ws.cap : 0u; }

// Calls body(first_entry, n_valid) for consecutive blocks of up to kBlock entries of the scope;
// every thread of the workgroup makes the same calls (collectives inside the body are allowed).
template <class F>
__device__ __forceinline__ void for_each_unit_block(const WaveSpace& ws, F&& body) {
    const uint32_t n_units = counted(ws, kCntUnits);
    for (uint32_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        const uint32_t base = ws.units[u].w;
        const uint32_t count = ws.unit_hits[u];
        for (uint32_t k0 = 0; k0 < count; k0 += kBlock) body(base + k0, min(static_cast<uint32_t>(kBlock), count - k0));
    }
}
template <class F>
__device__ __forceinline__ void for_each_dense_block(uint32_t base, uint32_t count, F&& body) {
    for (uint32_t k0 = blockIdx.x * kBlock; k0 < count; k0 += gridDim.x * kBlock) body(base + k0, min(static_cast<uint32_t>(kBlock), count - k0));
}
template <class F>
__device__ __forceinline__ void for_each_entry_block(const WaveSpace& ws, Scope s, F&& body) {
    if (s.units()) for_each_unit_block(ws, body);
    if (s.dense()) for_each_dense_block(dense_base(ws, s), dense_count(ws, s), body);
}
// True when this workgroup will get no entry block of the scope: it can leave before it stages the scene
// tables (a deep level holds a few thousand entries, yet every workgroup of a launch would stage 8.7 KB).
__device__ __forceinline__ bool no_entry_blocks(const WaveSpace& ws, Scope s) {
    if (s.units() && blockIdx.x < counted(ws, kCntUnits)) return false;
    if (s.dense() && static_cast<unsigned long long>(blockIdx.x) * kBlock < dense_count(ws, s)) return false;
    return true;
}

struct Record {
    Ray ray;
    Hit hit;
    uint32_t root;
    int depth;
};
__device__ __forceinline__ Record load_record(const WaveSpace& ws, int par, uint32_t e, bool with_texel) {
    Record r;
    const float4 qo = ws.q_o[par][e], qd = ws.q_d[par][e], qp = ws.q_p[par][e], qn = ws.q_n[par][e];
    r.root = __float_as_uint(qo.w);
    r.depth = __float_as_int(qd.w);
    r.ray = Ray{mk(qo.x, qo.y, qo.z), mk(qd.x, qd.y, qd.z)};
    r.hit.hit = true;
    r.hit.outer = false;
    r.hit.t = 0.0f;
    r.hit.p = mk(qp.x, qp.y, qp.z);
    r.hit.n = mk(qn.x, qn.y, qn.z);
    r.hit.tex = C4{0.0f, 0.0f, 0.0f, 1.0f};
    if (with_texel) {
        const float4 qt = ws.q_t[par][e];
        r.hit.tex = C4{qt.x, qt.y, qt.z, qt.w};
    }
    return r;
}

// The S light sample positions of one hit: mt19937(shadow seed) → 2·S draws → disk samples
// (shading.cpp:28-53).  kGeneral: streams longer than 227 draws use the full engine in HBM.
template <bool kGeneral>
struct SampleRng {
    using type = MtShort;
};
template <>
struct SampleRng<true> {
    using type = HitRng;
};

// seeds the engine of one hit (the sequential part: the 397-step mt19937 recurrence)
template <bool kGeneral>
__device__ __forceinline__ void seed_light_rng(typename SampleRng<kGeneral>::type& rng, V3 P, int depth, int S, uint32_t* my_rng) {
    if constexpr (kGeneral)
        rng.seed(shadow_seed(P, depth), 2 * S, my_rng);
    else
        rng.seed(shadow_seed(P, depth));
}

// 2·S draws of a seeded engine → the S light sample positions of entry e
// ... and the hit's bundle mask: which meshes any of its S shadow rays can meet (rt::bundle_candidates)
template <bool kPosed, class Rng>
__device__ __forceinline__ void write_light_samples(const SceneView& sc, const WaveSpace& ws, uint32_t e, V3 P, V3 N, int S, Rng& rng) {
    ws.cand[e] = bundle_candidates<kPosed>(sc, P + N * 1e-3f, ld3(sc.hdr->light_pos), sc.hdr->light_radius);
    const LightFrame frame = light_frame(sc, P);
    float* dst = ws.targets + static_cast<size_t>(e) * 3 * S;
    for (int i = 0; i < S; ++i) {
        const float d0 = rng.uniform();
        const float d1 = rng.uniform();
        const V3 t = light_sample_on_frame(sc, frame, d0, d1);
        dst[3 * i + 0] = t.x;
        dst[3 * i + 1] = t.y;
        dst[3 * i + 2] = t.z;
    }
}

template <bool kGeneral, bool kPosed>
__device__ __forceinline__ void emit_light_samples(const SceneView& sc, const float4* __restrict__ sample_table, const WaveSpace& ws, uint32_t e, V3 P, V3 N,
                                                   int depth, int S, uint32_t* my_rng) {
    if (sample_row_positions(sc, sample_table, shadow_seed(P, depth), P, S, ws.targets + static_cast<size_t>(e) * 3 * S)) {  // the seed's row of the device's table
        ws.cand[e] = bundle_candidates<kPosed>(sc, P + N * 1e-3f, ld3(sc.hdr->light_pos), sc.hdr->light_radius);
        return;
    }
    typename SampleRng<kGeneral>::type rng;
    seed_light_rng<kGeneral>(rng, P, depth, S, my_rng);
    write_light_samples<kPosed>(sc, ws, e, P, N, S, rng);
}

// light_samples: per record, the 397-step mt19937 seeding recurrence (sequential), then its 2·S
// draws turned into the S light sample positions.  One record per lane: thousands of resident waves
// hide the integer chain, and the S independent cos/sin/sqrt evaluations of a hit interleave.
template <bool kGeneral, bool kPosed>
__global__ __launch_bounds__(kBlock) void light_samples_kernel(const uint8_t* __restrict__ scene_blob, const RenderParams p,
                                                               const int level) {
    const SceneView sc = view_of(scene_blob);
    const WaveSpace& ws = p.ws;
    const Scope scope{level, p.flat};
    const int par = scope.par();
    const int S = p.cfg.shadow_samples;
    uint32_t* my_rng = nullptr;
    if constexpr (kGeneral)
        my_rng = ws.hit_rng + (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x) * 624;
    for_each_entry_block(ws, scope, [&](uint32_t first, uint32_t n) __attribute__((always_inline)) {
        if (threadIdx.x >= n) return;
        const uint32_t e = first + threadIdx.x;
        const float4 hp = ws.q_p[par][e], hn = ws.q_n[par][e];
        emit_light_samples<kGeneral, kPosed>(sc, p.sample_table, ws, e, mk(hp.x, hp.y, hp.z), mk(hn.x, hn.y, hn.z), __float_as_int(ws.q_d[par][e].w), S,
                                             my_rng);
    });
}

// shadow: one (record, light sample) pair per lane
// occupancy targets of the queue kernels (measured: 5 waves/SIMD best for shadow; 6+ spills)
#ifndef MCRT_SHADOW_WAVES
#define MCRT_SHADOW_WAVES 5
#endif
template <int kView>
__global__ __launch_bounds__(kBlock, MCRT_SHADOW_WAVES) void shadow_kernel(const uint8_t* __restrict__ scene_blob, const RenderParams p,
                                                        const int level) {
    extern __shared__ __align__(16) unsigned char s_dyn[];
    const SceneView scg = view_of(scene_blob);
    const WaveSpace& ws = p.ws;
    const Scope scope{level, p.flat};
    const int par = scope.par();
    const int mode = shadow_mode(scg, p.cfg);
    const int S = p.cfg.shadow_samples;
    const uint32_t pairs_per_hit = (mode == SHADOW_SOFT) ? static_cast<uint32_t>(S) : 1u;
    // groups of pairs_per_hit consecutive lanes belong to one hit; when that is a power of two
    // <= 64 the lit count is a ballot + popcount, otherwise atomics on a zeroed counter
    const bool pow2 = (pairs_per_hit & (pairs_per_hit - 1u)) == 0u && pairs_per_hit <= 64u;
    const uint32_t n_dense = scope.dense() ? dense_count(ws, scope) : 0u;
    {  // leave before the collective staging when this workgroup gets nothing
        const bool some_units = scope.units() && blockIdx.x < counted(ws, kCntUnits);
        const unsigned long long dense_items = pow2 ? static_cast<unsigned long long>(n_dense) * pairs_per_hit : n_dense;  // pow2: strided over pairs
        if (!some_units && static_cast<unsigned long long>(blockIdx.x) * kBlock >= dense_items) return;
    }
    const typename ViewSel<kView>::type sc = ViewSel<kView>::make(scg, p, s_dyn);
    uint32_t* lit = ws.lit[par];
    const V3 lpos = ld3(sc.hdr->light_pos);
    const uint32_t lane = threadIdx.x & 63u;
    // one wave-aligned group of up to 64 consecutive (entry, sample) pairs of the range `first` .. +total
    auto trace_pairs = [&](uint32_t first, uint32_t q0, uint32_t total) __attribute__((always_inline)) {
        const uint32_t q = q0 + lane;
        bool visible = false;
        uint32_t e = 0;
        if (q < total) {
            const uint32_t k = q / pairs_per_hit;
            const uint32_t j = q - k * pairs_per_hit;
            e = first + k;
            const float4 hp = ws.q_p[par][e], hn = ws.q_n[par][e];
            const V3 P = mk(hp.x, hp.y, hp.z);
            V3 N = mk(hn.x, hn.y, hn.z);
            if (mode == SHADOW_HARD) N = normalize(N);
            V3 target = lpos;
            if (mode == SHADOW_SOFT) {  // the first pass was done once for the hit's whole bundle of rays
                target = ld3(ws.targets + (static_cast<size_t>(e) * S + j) * 3);
                visible = !in_shadow_masked(sc, P, N, target, ws.cand[e]);
            } else {
                visible = !in_shadow_inline(sc, P, N, target);
            }
        }
        if (pow2) {
            const unsigned long long m = __ballot(visible);
            if (q < total && (lane & (pairs_per_hit - 1u)) == 0u) {
                const unsigned long long grp =
                    (pairs_per_hit == 64u) ? m : ((m >> lane) & ((1ull << pairs_per_hit) - 1ull));
                lit[e] = static_cast<uint32_t>(__popcll(grp));
            }
        } else if (visible) {
            atomicAdd(&lit[e], 1u);
        }
    };
    auto entry_block = [&](uint32_t first, uint32_t n) __attribute__((always_inline)) {
        if (!pow2) {
            if (threadIdx.x < n) lit[first + threadIdx.x] = 0u;
            __syncthreads();
        }
        const uint32_t total = n * pairs_per_hit;
        // every lane of a wave runs the same number of iterations (ballot inside)
        for (uint32_t q0 = threadIdx.x & ~63u; q0 < total; q0 += kBlock) trace_pairs(first, q0, total);
    };
    if (scope.units()) for_each_unit_block(ws, entry_block);
    if (!scope.dense()) return;
    const uint32_t base = dense_base(ws, scope);
    if (pow2) {
        // dense queue: stride over PAIRS so that even a sparse queue spreads over all workgroups
        const unsigned long long total = static_cast<unsigned long long>(n_dense) * pairs_per_hit;
        const unsigned long long step = static_cast<unsigned long long>(gridDim.x) * kBlock;
        for (unsigned long long q0 = static_cast<unsigned long long>(blockIdx.x) * kBlock + (threadIdx.x & ~63u); q0 < total; q0 += step) {
            // 64 consecutive pairs start at entry q0 / pairs_per_hit exactly (pairs_per_hit divides 64)
            const uint32_t first = base + static_cast<uint32_t>(q0 / pairs_per_hit);
            const uint32_t left = static_cast<uint32_t>(min(total - q0, 64ull));
            trace_pairs(first, 0u, left);
        }
    } else {
        for_each_dense_block(base, n_dense, entry_block);
    }
}

// ---------------------------------------------------------------------------------------------
// lit (flat pipeline): light samples, shadow rays AND shading of every record in one launch, handed over
// through LDS.  Per block of up to `lit_round` records:
//   phase A  a lane per record — the 397-step mt19937 seeding recurrence, the 2·S draws, the S disk
//            sample positions and the record's bundle mask (shading.cpp:28-53) — into LDS;
//   phase B  a lane per (record, light sample) — the exact any-hit test on the bundle mask — lit
//            count by ballot (S a power of two) or LDS atomics, into LDS;
//   phase C  a lane per record — Blinn-Phong with that visibility term (shading.cpp:62-96), times the AO
//            factor for primary hits (raytracer.cpp:121-130; the AO stage runs before this kernel) — onto
//            the chain's stack at the record's depth.
// As separate kernels the positions and masks went through HBM (96 + 8 B written and read back per
// record: ~180 MB of the metric frame's counted traffic), and the VALU-bound seeding chains could not
// overlap the latency-bound shadow rays.  Hard shadows / a point light: no phase A, one ray per record.
// ---------------------------------------------------------------------------------------------
#ifndef MCRT_LIT_WAVES
#define MCRT_LIT_WAVES 4
#endif
// What `lit`'s phases read of the shadow configuration, and the workgroup's LDS area behind the scene tables.  Five scalars
// (LitKnobs) live across the work-item loop; a phase forms the rest from them where it begins, by scalar arithmetic alone —
// no load, no wait.  (Formed from the parameters in every phase, with the light's radius from the scene header, a round
// waited eight times for scalar loads behind its barriers: `lit` spilled less still, and the 4K workload lost 2 % of its
// throughput — profiles/sgpr_spills/README.md, "Measured and rejected".)
struct LitKnobs {
    int mode, S, lds_offset;
    uint32_t round, pass;
    __device__ __forceinline__ LitKnobs(const SceneView& scg, const RenderParams& p)
        : mode(shadow_mode(scg, p.cfg)), S(p.cfg.shadow_samples), lds_offset(p.lit_lds_offset), round(static_cast<uint32_t>(p.lit_round)),
          pass(static_cast<uint32_t>(p.lit_pass)) {}  // pass: records whose sample positions fit the LDS area at once
};
struct LitShape {
    int mode, S;
    uint32_t pairs_per_hit;
    bool pow2;
    unsigned long long* s_cand;
    unsigned long long* s_ins;  // of the candidates, the boxes that hold the record's ray origin strictly inside (rt::mesh_candidate_inside)
    float* s_pos;
    uint32_t* s_lit;
    uint32_t* s_und;  // the round's undecided records, packed
    __device__ __forceinline__ LitShape(const LitKnobs& k, unsigned char* s_dyn) {
        int off = k.lds_offset;
        asm volatile("" : "+s"(off));  // formed here, not once above the loop and carried
        mode = k.mode;
        S = k.S;
        pairs_per_hit = (mode == SHADOW_SOFT) ? static_cast<uint32_t>(S) : 1u;
        pow2 = (pairs_per_hit & (pairs_per_hit - 1u)) == 0u && pairs_per_hit <= 64u;
        s_cand = reinterpret_cast<unsigned long long*>(s_dyn + off);  // 16-aligned
        s_ins = s_cand + k.round;
        s_pos = reinterpret_cast<float*>(s_ins + k.round);
        s_lit = reinterpret_cast<uint32_t*>(s_pos + static_cast<size_t>(k.pass) * pairs_per_hit * 3);
        s_und = s_lit + k.round;
    }
};
template <int kView>
__device__ __forceinline__ void lit_body(const uint8_t* __restrict__ scene_blob, const ParamPtr pp) {
    extern __shared__ __align__(16) unsigned char s_dyn[];  // [scene tables][candidate masks: lit_round][inside masks: lit_round][positions: lit_pass x S x 3 floats][lit counts: lit_round][undecided list: lit_round]
    __shared__ int s_wcnt[kBlock / 64];
    __shared__ uint32_t s_ticket[2];
    MCRT_HOOK_LIT_SHARED
    // The parameters by phase (kernel_common.h, phase_params): across the work-item loop live the list's counts, the scene
    // view and `pp`.
    const SceneView scg = view_of(scene_blob);
    const RenderParams& p = phase_params(pp);  // ---- entry: the work list
    const WaveSpace& ws = p.ws;
    const Scope scope{0, 1};
    // ONE work list — the units' record ranges, then the dense queue in blocks of 256 — so that the three phases
    // exist once in the code object (inlined per list they made 33 KB, half the instruction cache)
    const uint32_t n_units = counted(ws, kCntUnits);
    const uint32_t n_dense = dense_count(ws, scope);
    const uint32_t n_items = n_units + (n_dense + kBlock - 1u) / kBlock;
    // The chase: the chains below the level-1 records are followed HERE, ahead of the work list — a block of 256
    // level-1 records per workgroup turn, a lane per chain — and the records they append (levels >= 2) go to a region
    // of the dense queue that belongs to that block alone: no global counter, and no other workgroup ever waits for
    // them.  The workgroup that made them lights and shades them itself, as one more (sparse) entry of its work list.
    // (As a launch of its own between `primary` and `lit` the chase was 32 us of a lone frame's 225 for 2 us of work —
    // three dependent scene queries on 122 workgroups; in here it costs `lit` 5.)
    const int max_b = p.cfg.max_bounces;
    const uint32_t count1 = counted(ws, kCntDeep1);
    const uint32_t n_chase = max_b >= 1 ? (count1 + kBlock - 1u) / kBlock : 0u;
    const uint32_t n_work = n_chase + n_items;
    if (blockIdx.x >= n_work) return;  // before the collective staging
    const typename ViewSel<kView>::type sc = ViewSel<kView>::make(scg, p, s_dyn);
    constexpr bool kPosed = kView != kViewLdsUnposed;
    const LitKnobs knobs(scg, p);
    const uint32_t lane = threadIdx.x & 63u;
    // (the list by ticket: next_work; its order — chase blocks, units, dense blocks — puts the dearest items first)
    uint32_t turn = 0;
    for (uint32_t work = blockIdx.x; work < n_work; work = next_work(phase_params(pp), kCntTicketLit, work, n_work, s_ticket, turn)) {
        uint32_t first, n;
        // ---- phase: the work item — a chase block, a unit's records or a block of the dense queue
        const RenderParams& p = phase_params(pp);
        const WaveSpace& ws = p.ws;
        const bool posed = kView != kViewLdsUnposed && p.scene_posed != 0;  // the un-posed variants never read q_n
        if (work < n_chase) {
            // the chains of level-1 records [k0, k0 + 256): a lane per chain — reflect, closest hit, append — until the ray
            // misses or the chain reaches maxBounces; ~10 % of the lanes go on per turn, the loop is workgroup-uniform
            const uint32_t k0 = work * kBlock;
            const uint32_t region = ws.cap + n_chase * kBlock + k0 * static_cast<uint32_t>(max_b - 1);  // 256 x (maxBounces - 1) slots per block
            uint32_t filled = 0;  // uniform
            bool active = k0 + threadIdx.x < count1;
            RecordGeom r;
            r.root = 0;
            r.depth = 1;
            r.d = mk(0, 0, 0);
            r.p = mk(0, 0, 0);
            r.n = mk(0, 0, 0);
            if (active) r = load_geom(ws, posed, ws.cap + k0 + threadIdx.x);
            for (;;) {
                bool next_hit = false;
                Ray nray{mk(0, 0, 0), mk(0, 0, 0)};
                Hit nhit;
                nhit.hit = false;
                if (active) {
                    if (r.depth >= max_b) {  // no reflection at the last level
                        phase_params(pp).ws.end[r.root] = chain_code(r.depth + 1, true);
                        active = false;
                    } else {
                        nray = reflect_ray(r.d, r.p, r.n);
                        nhit = hit_scene<true>(sc, nray, ~0ull);
                        if (nhit.hit) {
                            next_hit = true;
                        } else {
                            phase_params(pp).ws.end[r.root] = chain_code(r.depth + 1, false);
                            active = false;
                        }
                    }
                }
                int total = 0;
                const int rank = block_rank(next_hit, s_wcnt, total);
                if (total == 0) break;  // uniform: no chain of this block goes on
                if (next_hit) {
                    push_record(phase_params(pp).ws, posed, region + filled + static_cast<uint32_t>(rank), nray, nhit, r.root, r.depth + 1, true);
                    r.d = nray.d;
                    r.p = nhit.p;
                    r.n = nhit.n;
                    ++r.depth;
                }
                filled += static_cast<uint32_t>(total);
            }
            __syncthreads();  // the block's own records, written by other lanes than the ones that read them below
            first = region;
            n = filled;
        } else if (work - n_chase < n_units) {
            first = ws.units[work - n_chase].w;
            n = ws.unit_hits[work - n_chase];
        } else {
            const uint32_t k0 = (work - n_chase - n_units) * kBlock;
            first = ws.cap + k0;
            n = min(static_cast<uint32_t>(kBlock), n_dense - k0);
        }
        const uint32_t round = knobs.round;
        for (uint32_t r0 = 0; r0 < n; r0 += round) {  // uniform
            const uint32_t m = min(round, n - r0);
            const uint32_t base = first + r0;
            uint32_t n_und = m;  // records whose rays are traced
            {
                // ---- phase A1: a lane per record — the bundle mask, and whether the whole bundle is decided (rt::bundle_classify)
                const RenderParams& p = phase_params(pp);
                const LitShape ls(knobs, s_dyn);
                bool undecided = false;
                if (threadIdx.x < m) {
                    if (ls.mode == SHADOW_SOFT) {
                        const RecordGeom g = load_geom(p.ws, kView != kViewLdsUnposed && p.scene_posed != 0, base + threadIdx.x);
                        const V3 O = g.p + g.n * 1e-3f;
                        const V3 lpos = ld3(scg.hdr->light_pos);
                        const float lradius = scg.hdr->light_radius;
                        unsigned long long cand;
                        const int known = bundle_classify<kPosed>(scg, sc, O, lpos, lradius, ls.S, p.bundle_decisions != 0, cand);
                        undecided = known < 0;
                        MCRT_HOOK_LIT_CLASSIFIED(known, undecided, cand, O)
                        ls.s_cand[threadIdx.x] = cand;
                        ls.s_ins[threadIdx.x] = (undecided && p.inside_fast) ? origin_inside_boxes(sc, O, cand) : 0ull;
                        ls.s_lit[threadIdx.x] = undecided ? 0u : static_cast<uint32_t>(known);
                    } else {
                        ls.s_lit[threadIdx.x] = 0u;
                    }
                }
                if (ls.mode == SHADOW_SOFT) {
                    int total = 0;
                    const int rank = block_rank(undecided, s_wcnt, total);
                    if (undecided) ls.s_und[rank] = threadIdx.x;
                    n_und = static_cast<uint32_t>(total);
                    if (n_und == 0u) {  // uniform: no ray of this round needs tracing
                        __syncthreads();
                        goto shade_round;
                    }
                    __syncthreads();
                }
            }
            // the traced records in passes of up to `pass` (their sample positions share the LDS area: with the
            // bundle decisions few records of a round are left, and the area is sized for those)
            for (uint32_t u0 = 0, pass = knobs.pass; u0 < n_und; u0 += pass) {  // uniform
                const uint32_t nu = min(pass, n_und - u0);
                if (u0) __syncthreads();  // the previous pass's rays have read the positions
                {
                    // ---- phase A2: a lane per undecided record — its mt19937 stream and the S disk sample positions
                    const RenderParams& p = phase_params(pp);
                    const LitShape ls(knobs, s_dyn);
                    if (ls.mode == SHADOW_SOFT && threadIdx.x < nu) {
                        const RecordGeom g = load_geom(p.ws, kView != kViewLdsUnposed && p.scene_posed != 0, base + ls.s_und[u0 + threadIdx.x]);
                        disk_sample_positions(scg, p.sample_table, p.seed_table, p.seed_table_full, g.p, g.depth, ls.S, ls.s_pos + static_cast<size_t>(threadIdx.x) * 3 * ls.S);
                    }
                }
                __syncthreads();
                // ---- phase B: a lane per (undecided record, light sample); every lane of a wave runs the same number of turns (ballot inside)
                const RenderParams& p = phase_params(pp);
                const LitShape ls(knobs, s_dyn);
                const bool posed = kView != kViewLdsUnposed && p.scene_posed != 0;
                const uint32_t total = nu * ls.pairs_per_hit;
                for (uint32_t q0 = threadIdx.x & ~63u; q0 < total; q0 += kBlock) {
                    const uint32_t q = q0 + lane;
                    bool visible = false;
                    uint32_t k = 0;
                    if (q < total) {
                        const uint32_t j = u0 + q / ls.pairs_per_hit;
                        k = (ls.mode == SHADOW_SOFT) ? ls.s_und[j] : j;
                        V3 P, N;
                        load_point_normal(p.ws, posed, base + k, P, N);
                        if (ls.mode == SHADOW_HARD) N = normalize(N);
                        if (ls.mode == SHADOW_SOFT)
                            visible = !in_shadow_masked(sc, P, N, ld3(ls.s_pos + static_cast<size_t>(q) * 3), ls.s_cand[k], ls.s_ins[k]);
                        else
                            visible = !in_shadow_inline(sc, P, N, ld3(scg.hdr->light_pos));
                    }
                    if (ls.pow2) {
                        const unsigned long long bal = __ballot(visible);
                        if (q < total && (lane & (ls.pairs_per_hit - 1u)) == 0u) {
                            const unsigned long long grp = (ls.pairs_per_hit == 64u) ? bal : ((bal >> lane) & ((1ull << ls.pairs_per_hit) - 1ull));
                            ls.s_lit[k] = static_cast<uint32_t>(__popcll(grp));
                        }
                    } else if (visible) {
                        atomicAdd(&ls.s_lit[k], 1u);
                    }
                }
            }
            __syncthreads();  // the counts are complete; the next round may overwrite the positions
        shade_round:
            // ---- phase C: a lane per record
            if (threadIdx.x < m) {
                const RenderParams& p = phase_params(pp);
                const WaveSpace& ws = p.ws;
                const mcrt_config& cfg = p.cfg;
                const LitShape ls(knobs, s_dyn);
                const int mode = ls.mode;
                const uint32_t e = base + threadIdx.x;
                const RecordGeom r = load_geom(ws, kView != kViewLdsUnposed && p.scene_posed != 0, e);
                Hit hit;
                hit.hit = true;
                hit.p = r.p;
                hit.n = r.n;
                hit.tex = texel_color(scg, ws.q_x[e]);  // the colour of the face's texel, from the pool
                V3 origin = ld3(scg.hdr->cam_pos);
                if (r.depth > 0 || (cfg.dof_enabled && cfg.aperture > 1e-6f)) {
                    const float4 qo = ws.q_o[0][e];
                    origin = mk(qo.x, qo.y, qo.z);
                }
                const uint32_t lit = ls.s_lit[threadIdx.x];
                MCRT_HOOK_LIT_SHADED(lit, r)
                const float vis = (mode == SHADOW_SOFT) ? static_cast<float>(lit) / static_cast<float>(ls.S) : (lit ? 1.0f : 0.0f);
                C4 c = shade(scg, hit, normalize(origin - hit.p), vis);
                if (cfg.ao_enabled && r.depth == 0) {  // occluded count from the ao stage (e < cap: a primary hit)
                    const float ao = 1.0f - static_cast<float>(ws.lit[1][e]) / static_cast<float>(cfg.ao_samples);
                    const float kk = 1.0f - cfg.ao_intensity * (1.0f - ao);
                    c.r *= kk;
                    c.g *= kk;
                    c.b *= kk;
                }
                ws.stack[static_cast<size_t>(r.depth) * ws.cap + r.root] = make_float4(c.r, c.g, c.b, c.a);  // plane-major: [depth][sample slot]
            }
        }
    }
}
template <int kView>
__global__ __launch_bounds__(kBlock, MCRT_LIT_WAVES) void lit_kernel(const RenderParams p, const uint8_t* __restrict__ scene_blob) {
    lit_body<kView>(scene_blob, kernarg_params());
}

// ambient occlusion (raytracer.cpp:38-78, depth 0 only) as one stage over the primary hits, a lane per hit:
//   1. the meshes any of its rays can meet: within the radius (rt::ball_candidates) and not behind the hit's own
//      face (the rays leave into the hemisphere around the normal; for an axis-aligned normal the tangent frame
//      is made of exact axis vectors, so the component of every direction along the normal is >= 0 and a box that
//      ends before the origin on that axis is missed by the moving-away argument of rt::bundle_decide_mesh);
//   2. hits with no such mesh are done (0 occluded) — the others are packed onto the block's first lanes;
//   3. per packed lane: mt19937(ao seed), and for each of the A directions the two draws, the cosine-weighted
//      direction and the any-hit test, counted in a register.
// (As two kernels — directions to HBM a lane per hit, rays a lane per (hit, direction) — the stage moved
// 2 x 192 B per hit through HBM with 64 cache lines per store instruction, and every ray lane reloaded and
// re-normalised its hit: 5.7 ms of the reference GUI's default frame; see DESIGN.md.)
#ifndef MCRT_AO_WAVES
#define MCRT_AO_WAVES 4
#endif
template <int kView>
__device__ __forceinline__ void ao_body(const uint8_t* __restrict__ scene_blob, const ParamPtr pp) {
    __shared__ int s_wcnt[kBlock / 64];
    __shared__ uint32_t s_list[kBlock];
    __shared__ unsigned long long s_mask[kBlock];
    extern __shared__ __align__(16) unsigned char s_dyn[];
    // The parameters by phase (kernel_common.h, phase_params): the two halves of a block of hits read them where they begin
    const SceneView scg = view_of(scene_blob);
    if (blockIdx.x >= counted(phase_params(pp).ws, kCntUnits)) return;
    const typename ViewSel<kView>::type sc = ViewSel<kView>::make(scg, phase_params(pp), s_dyn);
    constexpr bool kPosed = kView != kViewLdsUnposed;
    for_each_unit_block(phase_params(pp).ws, [&](uint32_t first, uint32_t n) __attribute__((always_inline)) {
        bool traced = false;
        if (threadIdx.x < n) {
            // ---- phase: the meshes the hit's hemisphere of rays can meet
            const RenderParams& p = phase_params(pp);
            const WaveSpace& ws = p.ws;
            const bool posed = kPosed && p.scene_posed != 0;
            const float radius = p.cfg.ao_radius;
            uint32_t* occ_out = ws.lit[1];
            const uint32_t e = first + threadIdx.x;
            V3 P, Nraw;
            load_point_normal(ws, posed, e, P, Nraw);
            const V3 N = normalize(Nraw);
            const unsigned long long cand = hemisphere_candidates<kPosed>(scg, P + N * 1e-3f, N, radius);
            s_mask[threadIdx.x] = cand;
            traced = cand != 0ull || scg.n_meshes > 64;  // meshes beyond the mask are tested per ray
            if (!traced) occ_out[e] = 0u;
        }
        int total = 0;
        const int rank = block_rank(traced, s_wcnt, total);
        if (traced) s_list[rank] = threadIdx.x;
        __syncthreads();
        if (static_cast<int>(threadIdx.x) < total) {
            // ---- phase: the packed hits' rays
            const RenderParams& p = phase_params(pp);
            const WaveSpace& ws = p.ws;
            const bool posed = kPosed && p.scene_posed != 0;
            const int A = p.cfg.ao_samples;
            const float radius = p.cfg.ao_radius;
            uint32_t* occ_out = ws.lit[1];
            const uint32_t k = s_list[threadIdx.x];
            const uint32_t e = first + k;
            V3 P, Nraw;
            load_point_normal(ws, posed, e, P, Nraw);
            const V3 N = normalize(Nraw);
            const V3 T = (__builtin_fabsf(N.x) < 0.9f) ? normalize(cross(mk(1, 0, 0), N)) : normalize(cross(mk(0, 1, 0), N));
            const V3 B = cross(N, T);
            const unsigned long long cand = s_mask[k];
            const V3 O = P + N * 1e-3f;
            const unsigned long long inside = p.inside_fast ? origin_inside_boxes(sc, O, cand) : 0ull;  // every ray of the hit starts there
            MtShort rng;
            const uint32_t seed = ao_seed(P);
            if (p.seed_table_full)
                rng.seed_known(seed, p.seed_table_full[seed]);  // mt[397] of this seed: one load instead of the 397-step recurrence
            else
                rng.seed(seed);
            uint32_t occluded = 0;
            for (int i = 0; i < A; ++i) {
                const float r1 = rng.uniform();
                const float r2 = rng.uniform();
                const float sinT = sqrt_pos(1.0f - r1);
                const float cosT = sqrt_pos(r1);
                float sn, cs;
                mcrt_sincosf(kTwoPi * r2, &sn, &cs);
                const V3 local = mk(sinT * cs, cosT, sinT * sn);
                const V3 world = normalize(T * local.x + N * local.y + B * local.z);
                if (any_hit_masked(sc, Ray{O, world}, radius, cand, inside)) ++occluded;
            }
            occ_out[e] = occluded;
        }
        __syncthreads();  // s_list, s_mask are reused by the next block of hits
    });
}
template <int kView>
__global__ __launch_bounds__(kBlock, MCRT_AO_WAVES) void ao_kernel(const RenderParams p, const uint8_t* __restrict__ scene_blob) {
    ao_body<kView>(scene_blob, kernarg_params());
}

// level_shade (general variants): colour of the level, reflection ray, closest hit of the next level →
// survivors to the queue of level + 1 with their light samples (packed); ended chains fold their level
// colours back to front and write the sample's colour.
template <int kView>
__global__ __launch_bounds__(kBlock, 2) void level_shade_kernel(const uint8_t* __restrict__ scene_blob, const RenderParams p,
                                                              const int level) {
    constexpr bool kGeneral = true;
    __shared__ int s_wcnt[kBlock / 64];
    __shared__ uint32_t s_out_base;
    __shared__ float4 s_np[kBlock], s_nn[kBlock];  // new hits handed to the packed threads
    extern __shared__ __align__(16) unsigned char s_dyn[];
    const SceneView scg = view_of(scene_blob);
    const WaveSpace& ws = p.ws;
    const Scope scope{level, 0};
    if (no_entry_blocks(ws, scope)) return;  // before the collective staging
    const typename ViewSel<kView>::type sc = ViewSel<kView>::make(scg, p, s_dyn);
    const mcrt_config& cfg = p.cfg;
    const int par = level & 1;
    const int mode = shadow_mode(sc, cfg);
    const int S = cfg.shadow_samples;
    const float* fb = sc.hdr->background;
    const C4 flat_bg{fb[0], fb[1], fb[2], fb[3]};
    uint32_t* my_rng = nullptr;
    if (ws.hit_rng) my_rng = ws.hit_rng + (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x) * 624;
    for_each_entry_block(ws, scope, [&](uint32_t first, uint32_t n) __attribute__((always_inline)) {
        bool next_hit = false;
        Ray nray{mk(0, 0, 0), mk(0, 0, 0)};
        Hit nhit;
        nhit.hit = false;
        uint32_t root = 0;
        int depth = 0;
        if (threadIdx.x < n) {
            const uint32_t e = first + threadIdx.x;
            const Record r = load_record(ws, par, e, true);
            root = r.root;
            depth = r.depth;
            const uint32_t lit = ws.lit[par][e];
            const float vis =
                (mode == SHADOW_SOFT) ? static_cast<float>(lit) / static_cast<float>(S) : (lit ? 1.0f : 0.0f);
            const C4 c = level_color(sc, cfg, r.ray.o, r.hit, depth, vis, my_rng);
            bool done = false;
            C4 tail = flat_bg;
            if (depth >= cfg.max_bounces) {  // no reflection: `shadedColor.a = originalAlpha; return clamp()`
                tail = clamp4(c);
                done = true;
            } else {
                nray = reflect_ray(r.ray, r.hit);
                nhit = hit_scene<true>(sc, nray, ~0ull);
                if (nhit.hit) {  // the chain goes on: its level colour waits on the stack for the fold
                    ws.stack[static_cast<size_t>(depth) * ws.cap + root] = make_float4(c.r, c.g, c.b, c.a);
                    next_hit = true;
                } else {  // bounced ray missed → flat background (raytracer.cpp:94-102), folded in at once (:143-147)
                    tail = fold_reflection(c, flat_bg);
                    done = true;
                }
            }
            if (done) {  // unwind the recursion: fold the shallower levels' colours back to front
                for (int d = depth - 1; d >= 0; --d) {
                    const float4 sd = ws.stack[static_cast<size_t>(d) * ws.cap + root];
                    tail = fold_reflection(C4{sd.x, sd.y, sd.z, sd.w}, tail);
                }
                ws.scol[root] = make_float4(tail.r, tail.g, tail.b, tail.a);
            }
        }
        // survivors → dense level+1 queue: one atomic per block
        int total = 0;
        const int rank = block_rank(next_hit, s_wcnt, total);
        if (total > 0) {  // uniform
            if (threadIdx.x == 0) s_out_base = count_add(ws, kCntDense + level + 1, static_cast<uint32_t>(total));
            const bool soft = mode == SHADOW_SOFT;
            if (next_hit && soft) {  // hand the new hit to thread `rank`: the survivors' work below runs packed
                s_np[rank] = make_float4(nhit.p.x, nhit.p.y, nhit.p.z, __int_as_float(depth + 1));
                s_nn[rank] = make_float4(nhit.n.x, nhit.n.y, nhit.n.z, 0.0f);
            }
            __syncthreads();
            if (next_hit) push_entry(ws, par ^ 1, s_out_base + static_cast<uint32_t>(rank), nray, nhit, root, depth + 1);
            // The new entries' light samples (seeding chain + S samples) and bundle masks.  Only a few lanes
            // per wave survive; threads 0 .. total-1 do it instead, so the chain runs in ceil(total / 64) waves.
            if (soft && static_cast<int>(threadIdx.x) < total) {
                const float4 np = s_np[threadIdx.x], nn = s_nn[threadIdx.x];
                emit_light_samples<kGeneral, kView != kViewLdsUnposed>(scg, p.sample_table, ws, s_out_base + threadIdx.x, mk(np.x, np.y, np.z), mk(nn.x, nn.y, nn.z),
                                                                       __float_as_int(np.w), S, my_rng);
            }
            __syncthreads();
        }
    });
}

// ---------------------------------------------------------------------------------------------
// Extra lights (mcrt.h, "extra lights"): the three stages of the general variants for a handle that carries M = K + 1 lights,
// light 0 the scene header's, lights 1 .. K the LightSet argument's.  Kernels of their own beside light_samples, shadow and
// level_shade, which stay exactly as they are.  A record's lights sit side by side: light k of entry e owns the S sample
// positions at targets[(e * M + k) * 3 * S], the bundle mask cand[e * M + k] and the count lit[par][e * M + k]
// (plan_workspace sizes the three arrays for M).  One seeding chain and one set of 2·S draws per record feed all M disks; a
// light whose radius is below 1e-4 has no disk: computeSoftShadow's single ray (shading.cpp:30) is traced by its sample 0.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ LightAt light_at(const FlatHeader* h, const LightSet& ls, uint32_t k) {
    // (selects, not an index: k differs from lane to lane in `shadow_lights`, and an indexed kernel argument goes through scratch)
    const mcrt_light_source& a = ls.extra[0];
    const mcrt_light_source& b = ls.extra[1];
    const mcrt_light_source& c = ls.extra[2];
    auto pick = [k](float x0, float x1, float x2, float x3) { return k == 0u ? x0 : (k == 1u ? x1 : (k == 2u ? x2 : x3)); };
    LightAt l;
    l.pos = mk(pick(h->light_pos[0], a.position[0], b.position[0], c.position[0]), pick(h->light_pos[1], a.position[1], b.position[1], c.position[1]),
               pick(h->light_pos[2], a.position[2], b.position[2], c.position[2]));
    l.radius = pick(h->light_radius, a.radius, b.radius, c.radius);
    for (int i = 0; i < 3; ++i) l.col[i] = pick(h->light_color[i], a.color[i], b.color[i], c.color[i]);
    return l;
}

// The light samples of one record for every disk light: the seeding chain and the 2·S draws once, then per light its frame,
// its bundle mask and its S positions.
template <bool kPosed>
__device__ __forceinline__ void emit_lights_samples(const SceneView& sc, const WaveSpace& ws, const LightSet& ls, uint32_t e, V3 P, V3 N, int depth, int S,
                                                    uint32_t* my_rng) {
    const uint32_t M = static_cast<uint32_t>(ls.n_extra) + 1u;
    HitRng rng;
    rng.seed(shadow_seed(P, depth), 2 * S, my_rng);
    LightAt light[kMaxLights];
    LightFrame frame[kMaxLights];
#pragma unroll
    for (uint32_t k = 0; k < static_cast<uint32_t>(kMaxLights); ++k) {  // (unrolled: the arrays stay in registers)
        light[k] = light_at(sc.hdr, ls, k);
        if (k >= M || light[k].radius < 1e-4f) continue;
        ws.cand[static_cast<size_t>(e) * M + k] = bundle_candidates<kPosed>(sc, P + N * 1e-3f, light[k].pos, light[k].radius);
        frame[k] = light_frame_at(light[k].pos, P);
    }
    for (int i = 0; i < S; ++i) {
        const float d0 = rng.uniform();
        const float d1 = rng.uniform();
#pragma unroll
        for (uint32_t k = 0; k < static_cast<uint32_t>(kMaxLights); ++k) {
            if (k >= M || light[k].radius < 1e-4f) continue;
            const V3 t = light_sample_at(light[k], frame[k], d0, d1);
            float* dst = ws.targets + ((static_cast<size_t>(e) * M + k) * static_cast<size_t>(S) + static_cast<size_t>(i)) * 3;
            dst[0] = t.x;
            dst[1] = t.y;
            dst[2] = t.z;
        }
    }
}
// whether any of the M lights has a disk (else no record needs samples)
__device__ __forceinline__ bool any_disk_light(const FlatHeader* h, const LightSet& ls) {
    bool any = !(h->light_radius < 1e-4f);
    for (int k = 0; k < ls.n_extra; ++k) any = any || !(ls.extra[k].radius < 1e-4f);
    return any;
}

template <bool kPosed>
__global__ __launch_bounds__(kBlock) void light_samples_lights_kernel(const uint8_t* __restrict__ scene_blob, const RenderParams p, const int level,
                                                                      const LightSet ls) {
    const SceneView sc = view_of(scene_blob);
    const WaveSpace& ws = p.ws;
    const Scope scope{level, 0};
    const int par = scope.par();
    const int S = p.cfg.shadow_samples;
    if (!any_disk_light(sc.hdr, ls)) return;
    uint32_t* my_rng = ws.hit_rng + (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x) * 624;
    for_each_entry_block(ws, scope, [&](uint32_t first, uint32_t n) __attribute__((always_inline)) {
        if (threadIdx.x >= n) return;
        const uint32_t e = first + threadIdx.x;
        const float4 hp = ws.q_p[par][e], hn = ws.q_n[par][e];
        emit_lights_samples<kPosed>(sc, ws, ls, e, mk(hp.x, hp.y, hp.z), mk(hn.x, hn.y, hn.z), __float_as_int(ws.q_d[par][e].w), S, my_rng);
    });
}

// shadow_lights: one (record, light, sample) triple per lane.  A *group* is the pairs_per_group consecutive lanes of one
// (record, light): group v = e * M + k, so `shadow`'s two ways of counting — ballot + popcount where the group size is a
// power of two <= 64, atomics on a zeroed counter otherwise — carry over with groups in the place of records.
template <int kView>
__global__ __launch_bounds__(kBlock, MCRT_SHADOW_WAVES) void shadow_lights_kernel(const uint8_t* __restrict__ scene_blob, const RenderParams p, const int level,
                                                                                  const LightSet ls) {
    extern __shared__ __align__(16) unsigned char s_dyn[];
    const SceneView scg = view_of(scene_blob);
    const WaveSpace& ws = p.ws;
    const Scope scope{level, 0};
    const int par = scope.par();
    const bool soft = p.cfg.soft_shadows && p.cfg.shadow_samples > 1;
    const int S = p.cfg.shadow_samples;
    const uint32_t M = static_cast<uint32_t>(ls.n_extra) + 1u;
    const uint32_t pairs_per_group = soft ? static_cast<uint32_t>(S) : 1u;
    const bool pow2 = (pairs_per_group & (pairs_per_group - 1u)) == 0u && pairs_per_group <= 64u;
    const uint32_t n_dense = scope.dense() ? dense_count(ws, scope) : 0u;
    {  // leave before the collective staging when this workgroup gets nothing
        const bool some_units = scope.units() && blockIdx.x < counted(ws, kCntUnits);
        const unsigned long long dense_items = pow2 ? static_cast<unsigned long long>(n_dense) * M * pairs_per_group : n_dense;  // pow2: strided over pairs
        if (!some_units && static_cast<unsigned long long>(blockIdx.x) * kBlock >= dense_items) return;
    }
    const typename ViewSel<kView>::type sc = ViewSel<kView>::make(scg, p, s_dyn);
    uint32_t* lit = ws.lit[par];
    const uint32_t lane = threadIdx.x & 63u;
    // one wave-aligned run of up to 64 consecutive pairs of the groups first_group .. : pairs q0 .. of `total`
    auto trace_pairs = [&](uint32_t first_group, uint32_t q0, uint32_t total) __attribute__((always_inline)) {
        const uint32_t q = q0 + lane;
        bool visible = false;
        uint32_t v = 0;
        if (q < total) {
            const uint32_t g = q / pairs_per_group;
            const uint32_t j = q - g * pairs_per_group;
            v = first_group + g;
            const uint32_t e = v / M;
            const LightAt l = light_at(sc.hdr, ls, v - e * M);
            const float4 hp = ws.q_p[par][e], hn = ws.q_n[par][e];
            const V3 P = mk(hp.x, hp.y, hp.z);
            const V3 N = mk(hn.x, hn.y, hn.z);
            if (!soft) {  // shade()'s own test, normalised normal
                visible = !in_shadow_inline(sc, P, normalize(N), l.pos);
            } else if (l.radius < 1e-4f) {  // computeSoftShadow's single ray, raw normal: sample 0 alone
                if (j == 0u) visible = !in_shadow_inline(sc, P, N, l.pos);
            } else {
                const V3 target = ld3(ws.targets + (static_cast<size_t>(v) * S + j) * 3);
                visible = !in_shadow_masked(sc, P, N, target, ws.cand[v]);
            }
        }
        if (pow2) {
            const unsigned long long m = __ballot(visible);
            if (q < total && (lane & (pairs_per_group - 1u)) == 0u) {
                const unsigned long long grp = (pairs_per_group == 64u) ? m : ((m >> lane) & ((1ull << pairs_per_group) - 1ull));
                lit[v] = static_cast<uint32_t>(__popcll(grp));
            }
        } else if (visible) {
            atomicAdd(&lit[v], 1u);
        }
    };
    auto entry_block = [&](uint32_t first, uint32_t n) __attribute__((always_inline)) {
        const uint32_t first_group = first * M, groups = n * M;
        if (!pow2) {
            for (uint32_t i = threadIdx.x; i < groups; i += kBlock) lit[first_group + i] = 0u;
            __syncthreads();
        }
        const uint32_t total = groups * pairs_per_group;
        // every lane of a wave runs the same number of iterations (ballot inside)
        for (uint32_t q0 = threadIdx.x & ~63u; q0 < total; q0 += kBlock) trace_pairs(first_group, q0, total);
    };
    if (scope.units()) for_each_unit_block(ws, entry_block);
    if (!scope.dense()) return;
    const uint32_t base = dense_base(ws, scope);
    if (pow2) {
        // dense queue: stride over PAIRS so that even a sparse queue spreads over all workgroups
        const unsigned long long total = static_cast<unsigned long long>(n_dense) * M * pairs_per_group;
        const unsigned long long step = static_cast<unsigned long long>(gridDim.x) * kBlock;
        for (unsigned long long q0 = static_cast<unsigned long long>(blockIdx.x) * kBlock + (threadIdx.x & ~63u); q0 < total; q0 += step) {
            // 64 consecutive pairs start at group q0 / pairs_per_group exactly (pairs_per_group divides 64)
            const uint32_t first_group = base * M + static_cast<uint32_t>(q0 / pairs_per_group);
            const uint32_t left = static_cast<uint32_t>(min(total - q0, 64ull));
            trace_pairs(first_group, 0u, left);
        }
    } else {
        for_each_dense_block(base, n_dense, entry_block);
    }
}

// colour of a hit level under M lights (mcrt.h): C + E_1 .. E_K left to right, clamped, then the AO factor of level_color
template <class SV>
__device__ __forceinline__ C4 level_color_lights(const SV& sc, const mcrt_config& cfg, const LightSet& ls, V3 ray_origin, const Hit& hit, int depth,
                                                 const uint32_t* lit, bool soft, uint32_t* mt_storage) {
    const V3 view = normalize(ray_origin - hit.p);
    const float S = static_cast<float>(cfg.shadow_samples);
    auto vis_of = [&](uint32_t k, float radius) { return (soft && !(radius < 1e-4f)) ? static_cast<float>(lit[k]) / S : (lit[k] ? 1.0f : 0.0f); };
    C4 c = shade(sc, hit, view, vis_of(0u, sc.hdr->light_radius));
    for (int k = 1; k <= ls.n_extra; ++k) {
        const LightAt l = light_at(sc.hdr, ls, static_cast<uint32_t>(k));
        const C4 e = shade_at(l, hit, view, 0.0f, vis_of(static_cast<uint32_t>(k), l.radius));
        c.r += e.r;
        c.g += e.g;
        c.b += e.b;
    }
    c = clamp4(c);
    if (cfg.ao_enabled && depth == 0) {  // raytracer.cpp:121-130
        const float ao = ambient_occlusion(sc, hit.p, hit.n, cfg.ao_samples, cfg.ao_radius, ao_seed(hit.p), mt_storage);
        const float k = 1.0f - cfg.ao_intensity * (1.0f - ao);
        c.r *= k;
        c.g *= k;
        c.b *= k;
    }
    return c;
}

// level_shade_lights: level_shade with the level's colour summed over the lights and the next level's samples emitted for all of them
template <int kView>
__global__ __launch_bounds__(kBlock, 2) void level_shade_lights_kernel(const uint8_t* __restrict__ scene_blob, const RenderParams p, const int level,
                                                                     const LightSet ls) {
    __shared__ int s_wcnt[kBlock / 64];
    __shared__ uint32_t s_out_base;
    __shared__ float4 s_np[kBlock], s_nn[kBlock];  // new hits handed to the packed threads
    extern __shared__ __align__(16) unsigned char s_dyn[];
    const SceneView scg = view_of(scene_blob);
    const WaveSpace& ws = p.ws;
    const Scope scope{level, 0};
    if (no_entry_blocks(ws, scope)) return;  // before the collective staging
    const typename ViewSel<kView>::type sc = ViewSel<kView>::make(scg, p, s_dyn);
    const mcrt_config& cfg = p.cfg;
    const int par = level & 1;
    const bool soft = cfg.soft_shadows && cfg.shadow_samples > 1;
    const bool emit = soft && any_disk_light(scg.hdr, ls);
    const int S = cfg.shadow_samples;
    const uint32_t M = static_cast<uint32_t>(ls.n_extra) + 1u;
    const float* fb = sc.hdr->background;
    const C4 flat_bg{fb[0], fb[1], fb[2], fb[3]};
    uint32_t* my_rng = nullptr;
    if (ws.hit_rng) my_rng = ws.hit_rng + (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x) * 624;
    for_each_entry_block(ws, scope, [&](uint32_t first, uint32_t n) __attribute__((always_inline)) {
        bool next_hit = false;
        Ray nray{mk(0, 0, 0), mk(0, 0, 0)};
        Hit nhit;
        nhit.hit = false;
        uint32_t root = 0;
        int depth = 0;
        if (threadIdx.x < n) {
            const uint32_t e = first + threadIdx.x;
            const Record r = load_record(ws, par, e, true);
            root = r.root;
            depth = r.depth;
            const C4 c = level_color_lights(sc, cfg, ls, r.ray.o, r.hit, depth, ws.lit[par] + static_cast<size_t>(e) * M, soft, my_rng);
            bool done = false;
            C4 tail = flat_bg;
            if (depth >= cfg.max_bounces) {  // no reflection: `shadedColor.a = originalAlpha; return clamp()`
                tail = clamp4(c);
                done = true;
            } else {
                nray = reflect_ray(r.ray, r.hit);
                nhit = hit_scene<true>(sc, nray, ~0ull);
                if (nhit.hit) {  // the chain goes on: its level colour waits on the stack for the fold
                    ws.stack[static_cast<size_t>(depth) * ws.cap + root] = make_float4(c.r, c.g, c.b, c.a);
                    next_hit = true;
                } else {  // bounced ray missed → flat background (raytracer.cpp:94-102), folded in at once (:143-147)
                    tail = fold_reflection(c, flat_bg);
                    done = true;
                }
            }
            if (done) {  // unwind the recursion: fold the shallower levels' colours back to front
                for (int d = depth - 1; d >= 0; --d) {
                    const float4 sd = ws.stack[static_cast<size_t>(d) * ws.cap + root];
                    tail = fold_reflection(C4{sd.x, sd.y, sd.z, sd.w}, tail);
                }
                ws.scol[root] = make_float4(tail.r, tail.g, tail.b, tail.a);
            }
        }
        // survivors → dense level+1 queue: one atomic per block
        int total = 0;
        const int rank = block_rank(next_hit, s_wcnt, total);
        if (total > 0) {  // uniform
            if (threadIdx.x == 0) s_out_base = count_add(ws, kCntDense + level + 1, static_cast<uint32_t>(total));
            if (next_hit && emit) {  // hand the new hit to thread `rank`: the survivors' work below runs packed
                s_np[rank] = make_float4(nhit.p.x, nhit.p.y, nhit.p.z, __int_as_float(depth + 1));
                s_nn[rank] = make_float4(nhit.n.x, nhit.n.y, nhit.n.z, 0.0f);
            }
            __syncthreads();
            if (next_hit) push_entry(ws, par ^ 1, s_out_base + static_cast<uint32_t>(rank), nray, nhit, root, depth + 1);
            if (emit && static_cast<int>(threadIdx.x) < total) {  // the new entries' light samples and bundle masks, for every disk light
                const float4 np = s_np[threadIdx.x], nn = s_nn[threadIdx.x];
                emit_lights_samples<kView != kViewLdsUnposed>(scg, ws, ls, s_out_base + threadIdx.x, mk(np.x, np.y, np.z), mk(nn.x, nn.y, nn.z),
                                                              __float_as_int(np.w), S, my_rng);
            }
            __syncthreads();
        }
    });
}

// resolve: ordered per-pixel sum of the queued units' sample colours (tile_renderer.cpp:116-124).  A
// sample that started a chain gets its colour here: the chain's level colours folded back to front
// (raytracer.cpp:143-147) from where the chain ended — the flat background when its last reflection ray
// missed (:94-102), the clamped last level colour when it stopped at maxBounces (:146-147).
// A thread per SAMPLE fetches / folds the colour; the pixel's samples meet in LDS and one thread per
// pixel adds them in order (float addition order is part of the result).
// kTransparent (MCRT_BACKGROUND_TRANSPARENT, mcrt.h): a sample whose primary ray missed (kEndMiss) adds nothing and is not
// counted — its colour is never formed, so the tile's draws are not read here at all — and the pixel is (0,0,0,0) without a
// hit, else rgb · (1.0f / hits) and alpha · (1.0f / spp).  Both reciprocals are IEEE divisions (hipcc's default correctly
// rounded fp32 divide, like inv_spp).  A template parameter, not a field test: the reference instantiation is the kernel
// as it was, registers and LDS included.
template <bool kTransparent>
struct ResolveLds {
    float4 col[kBlock];
};
template <>
struct ResolveLds<true> {
    float4 col[kBlock];
    uint8_t hit[kBlock];  // the sample's primary ray hit
};
__device__ __forceinline__ float4 sample_colour(const WaveSpace& ws, uint32_t slot, uint32_t code, const C4& flat_bg) {
    if (code == 0u) return ws.scol[slot];
    const float4* lv = ws.stack + slot;  // level d of the chain: lv[d * cap]
    const size_t plane = ws.cap;
    C4 tail = flat_bg;
    int dd = static_cast<int>(code >> 1) - 1;  // the chain's last record
    if (code & 1u) {
        const float4 last = lv[dd * plane];
        tail = clamp4(C4{last.x, last.y, last.z, last.w});
        --dd;
    }
    for (; dd >= 0; --dd) {
        const float4 sd = lv[dd * plane];
        tail = fold_reflection(C4{sd.x, sd.y, sd.z, sd.w}, tail);
    }
    return make_float4(tail.r, tail.g, tail.b, tail.a);
}
template <bool kTransparent>
__device__ __forceinline__ void resolve_body(const uint8_t* __restrict__ scene_blob, const float* __restrict__ tile_draws,
                                             float4* __restrict__ out_frame, uchar4* __restrict__ out8, const ParamPtr pp,
                                             const int tile_base) {
    __shared__ ResolveLds<kTransparent> s_lds;
    float4* s_col = s_lds.col;
    // The parameters by phase (kernel_common.h, phase_params): a unit reads what it needs of them where it begins; across
    // the unit loop live its count, the scene view and `pp`.
    const SceneView scg = view_of(scene_blob);
    uint32_t n_units;
    float frame_w, frame_h, inv_spp;  // formed once (vector-unit conversions and a division), kept as scalars
    {  // ---- entry
        const RenderParams& p = phase_params(pp);
        const WaveSpace& ws = p.ws;
        n_units = ws.frame_info[0];  // (not from the counters: this kernel moves their base)
        frame_w = uniform_float(static_cast<float>(p.cfg.width)), frame_h = uniform_float(static_cast<float>(p.cfg.height));
        inv_spp = uniform_float(1.0f / static_cast<float>(p.cfg.samples_per_pixel > 1 ? static_cast<uint32_t>(p.cfg.samples_per_pixel) : 1u));
        MCRT_HOOK_RESOLVE_BEGIN()
        if (blockIdx.x == 0) {  // the pass has counted everything: where the counters stand is the next pass's base
            for (int i = threadIdx.x; i < kCounterWords - 4; i += kBlock) ws.counter_base[i] = ws.counters[i];
        }
    }
    for (uint32_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        // ---- phase: the unit
        const RenderParams& p = phase_params(pp);
        const WaveSpace& ws = p.ws;
        const mcrt_config& cfg = p.cfg;
        const FrameDiv fd(frame_w, frame_h, p);
        const uint32_t dd = static_cast<uint32_t>(p.draws_per_sample);
        // the colour of sample `sidx` (stream order) of unit d: a miss from its jitter pair — the expressions of `primary`'s
        // sample loop (tile_renderer.cpp:93-114) — else the chain's fold
        auto unit_sample = [&](const uint4& d, const TileGeom& tg, const float* draws, uint32_t sidx, uint32_t spp_) __attribute__((always_inline)) -> float4 {
            const uint32_t slot = d.w + sidx;
            const uint32_t code = ws.end[slot];
            if (code != kEndMiss) return sample_colour(ws, slot, code, C4{scg.hdr->background[0], scg.hdr->background[1], scg.hdr->background[2], scg.hdr->background[3]});
            const uint32_t k = UDiv(spp_).div(sidx);  // pixel of the unit
            int lx, ly;
            unit_pixel(d, tg, k, lx, ly);
            const int px = tg.x + lx, py = tg.y + ly;
            float jx = 0.5f, jy = 0.5f;
            if (spp_ > 1u) {
                const float2 j = *reinterpret_cast<const float2*>(draws + (static_cast<size_t>(ly * tg.w + lx) * spp_ + (sidx - k * spp_)) * dd);  // dd is even: 8-byte aligned
                jx = j.x, jy = j.y;
            }
            const C4 c = background(scg, cfg, fd.u(static_cast<float>(px) + jx), fd.v(static_cast<float>(py) + jy));
            return make_float4(c.r, c.g, c.b, c.a);
        };
        const uint32_t spp = cfg.samples_per_pixel > 1 ? static_cast<uint32_t>(cfg.samples_per_pixel) : 1u;
        const uint32_t chunk_px = spp <= static_cast<uint32_t>(kBlock) ? static_cast<uint32_t>(kBlock) / spp : 0u;  // pixels per pass (0: a pixel per thread, serially)
        auto put_pixel = [&](const uint4& d, const TileGeom& tg, uint32_t k, float4 acc) __attribute__((always_inline)) {  // pixel k of unit d
            int lx, ly;
            unit_pixel(d, tg, k, lx, ly);
            const int row = (p.layout == MCRT_LAYOUT_PACKED) ? ((p.shard.pack_first + tg.owned_row * p.shard.pack_step) * cfg.tile_size + ly) : (tg.y + ly);
            store_pixel(out_frame, out8, static_cast<size_t>(row) * cfg.width + (tg.x + lx),
                        make_float4(acc.x * inv_spp, acc.y * inv_spp, acc.z * inv_spp, acc.w * inv_spp));
        };
        // transparent: the colour of a sample whose primary ray hit (else `hit` = false and nothing is formed)
        auto hit_sample = [&](const uint4& d, uint32_t sidx, bool& hit) __attribute__((always_inline)) -> float4 {
            const uint32_t slot = d.w + sidx;
            const uint32_t code = ws.end[slot];
            hit = code != kEndMiss;
            if (!hit) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            return sample_colour(ws, slot, code, C4{scg.hdr->background[0], scg.hdr->background[1], scg.hdr->background[2], scg.hdr->background[3]});
        };
        // transparent: the sum of the n samples that hit
        auto put_pixel_transparent = [&](const uint4& d, const TileGeom& tg, uint32_t k, float4 acc, uint32_t n) __attribute__((always_inline)) {
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (n > 0u) {
                const float inv_n = 1.0f / static_cast<float>(n);
                v = make_float4(acc.x * inv_n, acc.y * inv_n, acc.z * inv_n, acc.w * inv_spp);
            }
            int lx, ly;
            unit_pixel(d, tg, k, lx, ly);
            const int row = (p.layout == MCRT_LAYOUT_PACKED) ? ((p.shard.pack_first + tg.owned_row * p.shard.pack_step) * cfg.tile_size + ly) : (tg.y + ly);
            store_pixel(out_frame, out8, static_cast<size_t>(row) * cfg.width + (tg.x + lx), v);
        };
        const uint4 d = ws.units[u];
        const int tile = unit_tile(d);
        const TileGeom tg = tile_of(p, tile);
        const uint32_t pp0 = 0u, pp1 = unit_pixels(d);  // the unit's pixels, in its own order (unit_pixel)
        // the tile's draws: at its touched-tile number, or (all tiles' streams in HBM) at its index in the batch — as in `primary`
        const float* draws = tile_draws + static_cast<size_t>(p.draw_plate ? static_cast<uint32_t>(tg.frame_tile)
                                                              : p.bg_in_plan ? d.w / ws.tile_slots : static_cast<uint32_t>(tile - tile_base)) * ws.draws_stride;
        if (chunk_px == 0u) {
            for (uint32_t i = pp0 + threadIdx.x; i < pp1; i += kBlock) {
                float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if constexpr (kTransparent) {
                    uint32_t n = 0;
                    for (uint32_t s = 0; s < spp; ++s) {
                        bool hit;
                        const float4 c = hit_sample(d, (i - pp0) * spp + s, hit);
                        if (!hit) continue;
                        acc.x += c.x, acc.y += c.y, acc.z += c.z, acc.w += c.w;
                        ++n;
                    }
                    put_pixel_transparent(d, tg, i, acc, n);
                } else {
                    for (uint32_t s = 0; s < spp; ++s) {
                        const float4 c = unit_sample(d, tg, draws, (i - pp0) * spp + s, spp);
                        acc.x += c.x, acc.y += c.y, acc.z += c.z, acc.w += c.w;
                    }
                    put_pixel(d, tg, i, acc);
                }
            }
            continue;
        }
        for (uint32_t p0 = pp0; p0 < pp1; p0 += chunk_px) {  // uniform
            const uint32_t npx = min(chunk_px, pp1 - p0);
            if constexpr (kTransparent) {
                if (threadIdx.x < npx * spp) {
                    bool hit;
                    s_col[threadIdx.x] = hit_sample(d, (p0 - pp0) * spp + threadIdx.x, hit);
                    s_lds.hit[threadIdx.x] = hit ? 1 : 0;
                }
            } else {
                if (threadIdx.x < npx * spp) s_col[threadIdx.x] = unit_sample(d, tg, draws, (p0 - pp0) * spp + threadIdx.x, spp);
            }
            __syncthreads();
            if (threadIdx.x < npx) {
                float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if constexpr (kTransparent) {
                    uint32_t n = 0;
                    for (uint32_t s = 0; s < spp; ++s) {
                        if (!s_lds.hit[threadIdx.x * spp + s]) continue;
                        const float4 c = s_col[threadIdx.x * spp + s];
                        acc.x += c.x, acc.y += c.y, acc.z += c.z, acc.w += c.w;
                        ++n;
                    }
                    put_pixel_transparent(d, tg, p0 + threadIdx.x, acc, n);
                } else {
                    for (uint32_t s = 0; s < spp; ++s) {
                        const float4 c = s_col[threadIdx.x * spp + s];
                        acc.x += c.x, acc.y += c.y, acc.z += c.z, acc.w += c.w;
                    }
                    put_pixel(d, tg, p0 + threadIdx.x, acc);
                }
            }
            __syncthreads();
        }
    }
}
__global__ __launch_bounds__(kBlock) void resolve_kernel(const RenderParams p, const uint8_t* __restrict__ scene_blob, const float* __restrict__ tile_draws,
                                                         float4* __restrict__ out_frame, uchar4* __restrict__ out8, const int tile_base) {
    resolve_body<false>(scene_blob, tile_draws, out_frame, out8, kernarg_params(), tile_base);
}
__global__ __launch_bounds__(kBlock) void resolve_transparent_kernel(const RenderParams p, const uint8_t* __restrict__ scene_blob, float4* __restrict__ out_frame,
                                                                     uchar4* __restrict__ out8, const int tile_base) {
    resolve_body<true>(scene_blob, nullptr, out_frame, out8, kernarg_params(), tile_base);
}

// ---------------------------------------------------------------------------------------------
// batched entry points (mcrt_render_batch_device): one launch per stage for N frames, blockIdx.y = frame.  The entry
// reads its frame's RenderParams from a device-resident table — a wave-uniform address, so the fields come in with scalar
// loads — and runs the single-frame body.  Everything per frame stays per frame because it comes from those parameters:
// the workspace, the pass counters and their base, frame_info, the blockIdx.x == 0 duties and the grid-stride loops over
// gridDim.x.  A batch holds frames of one config that take one pass each (tile_base 0), so the tile count is common.
// ---------------------------------------------------------------------------------------------
// The table is declared in the constant address space (4), as the single-frame entries' kernel arguments are: memory the
// kernel cannot write, so the pointers read from it are known to be global ones (global_load / global_store with scalar
// bases, as in the single-frame kernels) instead of generic flat accesses.
using ParamTable = const __attribute__((address_space(4))) RenderParams*;
__device__ __forceinline__ const RenderParams& frame_params(ParamTable table) { return *(const RenderParams*)(table + blockIdx.y); }
__global__ __launch_bounds__(64) void seed_tiles_batch_kernel(ParamTable table, int n_tiles) {
    seed_tiles_body(frame_params(table), n_tiles);
}
__global__ __launch_bounds__(64 * kStreamWaves) void advance_tiles_batch_kernel(ParamTable table, int n_tiles) {
    advance_tiles_body(frame_params(table), n_tiles);
}
__global__ __launch_bounds__(64 * kStreamWaves) void plan_tiles_batch_kernel(ParamTable table, const int n_tiles) {
    const RenderParams& p = frame_params(table);
    plan_tiles_body(p.scene, p.tile_rng, p.ws.tile_draws, reinterpret_cast<float4*>(p.out), reinterpret_cast<uchar4*>(p.out8), p, 0, n_tiles);
}
__global__ __launch_bounds__(kBlock, MCRT_BG_WAVES) void background_batch_kernel(ParamTable table, const int n_tiles) {
    const RenderParams& p = frame_params(table);
    background_body(p.scene, p.ws.tile_draws, reinterpret_cast<float4*>(p.out), reinterpret_cast<uchar4*>(p.out8), p, 0, n_tiles);
}
template <int kView>
__global__ __launch_bounds__(kBlock, MCRT_PRIMARY_WAVES) void primary_batch_kernel(ParamTable table, const int n_tiles) {
    const RenderParams& p = frame_params(table);
    primary_body<kView>(p.scene, p.draw_plate ? p.draw_plate : p.ws.tile_draws, reinterpret_cast<float4*>(p.out), reinterpret_cast<uchar4*>(p.out8), table + blockIdx.y, 0, n_tiles);
}
template <int kView>
__global__ __launch_bounds__(kBlock, MCRT_AO_WAVES) void ao_batch_kernel(ParamTable table) {
    ao_body<kView>(frame_params(table).scene, table + blockIdx.y);
}
template <int kView>
__global__ __launch_bounds__(kBlock, MCRT_LIT_WAVES) void lit_batch_kernel(ParamTable table) {
    lit_body<kView>(frame_params(table).scene, table + blockIdx.y);
}
__global__ __launch_bounds__(kBlock) void resolve_batch_kernel(ParamTable table) {
    const RenderParams& p = frame_params(table);
    resolve_body<false>(p.scene, p.draw_plate ? p.draw_plate : p.ws.tile_draws, reinterpret_cast<float4*>(p.out), reinterpret_cast<uchar4*>(p.out8), table + blockIdx.y, 0);
}
__global__ __launch_bounds__(kBlock) void resolve_transparent_batch_kernel(ParamTable table) {
    const RenderParams& p = frame_params(table);
    resolve_body<true>(p.scene, nullptr, reinterpret_cast<float4*>(p.out), reinterpret_cast<uchar4*>(p.out8), table + blockIdx.y, 0);
}

// ---- host-side launchers (the planning that sizes them: render_plan.cpp) ----------------------------
template <int kView>
static void launch_levels(const RenderParams& p, hipStream_t stream, size_t dyn, const LightSet* lights) {
    const mcrt_config& c = p.cfg;
    const bool soft = soft_sampling(c);
    const int levels = c.max_bounces < 0 ? 0 : c.max_bounces + 1;
    if (levels < 1) return;
    constexpr bool posed = kView != kViewLdsUnposed;
    (void)soft;
    if (!p.flat) {  // general variants: one launch set per level; `level_shade` emits the light samples of the entries it appends
        const int grid = 256;
        if (lights && lights->n_extra > 0) {  // extra lights: the same sequence through the multi-light stages
            for (int L = 0; L < levels; ++L) {
                if (soft && L == 0) hipLaunchKernelGGL(light_samples_lights_kernel<posed>, dim3(grid), dim3(kBlock), 0, stream, p.scene, p, L, *lights);
                hipLaunchKernelGGL(shadow_lights_kernel<kView>, dim3(grid), dim3(kBlock), dyn, stream, p.scene, p, L, *lights);
                hipLaunchKernelGGL(level_shade_lights_kernel<kView>, dim3(grid), dim3(kBlock), dyn, stream, p.scene, p, L, *lights);
            }
            return;
        }
        for (int L = 0; L < levels; ++L) {
            if (soft && L == 0) hipLaunchKernelGGL((light_samples_kernel<true, posed>), dim3(grid), dim3(kBlock), 0, stream, p.scene, p, L);
            hipLaunchKernelGGL(shadow_kernel<kView>, dim3(grid), dim3(kBlock), dyn, stream, p.scene, p, L);
            hipLaunchKernelGGL(level_shade_kernel<kView>, dim3(grid), dim3(kBlock), dyn, stream, p.scene, p, L);
        }
        return;
    }
    const int ao_grid = p.grid_ao > 0 ? p.grid_ao : kQueueGrid, lit_grid = p.grid_lit > 0 ? p.grid_lit : kQueueGrid;
    if (c.ao_enabled && c.ao_samples > 0) {  // ahead of `lit`, whose last phase applies the AO factor
        hipLaunchKernelGGL(ao_kernel<kView>, dim3(ao_grid), dim3(kBlock), dyn, stream, p, p.scene);
    }
    hipLaunchKernelGGL(lit_kernel<kView>, dim3(lit_grid), dim3(kBlock), static_cast<size_t>(p.lit_lds_offset) + static_cast<size_t>(p.lit_lds_bytes), stream, p, p.scene);
}

hipError_t launch_seed_tiles(const RenderParams& p, hipStream_t stream) {
    const int n = owned_tiles(p);
    if (n <= 0 || p.draws_per_sample <= 0 || !p.tile_rng) return hipSuccess;
    hipLaunchKernelGGL(seed_tiles_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, p, n);
    if (p.stream_parts > 1) hipLaunchKernelGGL(advance_tiles_kernel, dim3((n + kStreamWaves - 1) / kStreamWaves), dim3(64 * kStreamWaves), 0, stream, p, n);
    return hipGetLastError();
}

hipError_t launch_render(const RenderParams& p, hipStream_t stream, const LaunchMarks* marks, const LightSet* lights) {
    const int n = owned_tiles(p);
    if (n <= 0) return hipSuccess;
    if (lights && lights->n_extra > 0 && (p.flat || lights->n_extra > MCRT_MAX_EXTRA_LIGHTS)) return hipErrorInvalidValue;  // (plan_workspace sizes the workspace for them)
    const size_t dyn = scene_table_bytes(p);
    float4* out = reinterpret_cast<float4*>(p.out);
    uchar4* out8 = reinterpret_cast<uchar4*>(p.out8);
    if (static_cast<size_t>(p.lit_lds_offset) != ((dyn + 15) & ~static_cast<size_t>(15))) return hipErrorInvalidValue;  // set by plan_workspace's caller
    for (int r0 = 0; r0 < p.shard.owned_rows; r0 += p.rows_per_batch) {
        const int rows = p.rows_per_batch < p.shard.owned_rows - r0 ? p.rows_per_batch : p.shard.owned_rows - r0;
        const int tile_base = r0 * p.shard.tiles_x;
        const int batch_tiles = rows * p.shard.tiles_x;
        hipError_t e = hipSuccess;  // (no counter memset: the counters run on, `resolve` moves their base)
        const float* draws = p.draw_plate ? p.draw_plate : p.ws.tile_draws;  // what `primary` and `resolve` read the touched tiles' draws from
        hipLaunchKernelGGL(plan_tiles_kernel, dim3((batch_tiles * (p.stream_waves > 0 ? p.stream_waves : 1) + kStreamWaves - 1) / kStreamWaves), dim3(64 * kStreamWaves), 0, stream,
                           p.scene, p.tile_rng, p.ws.tile_draws, out, out8, p, tile_base, batch_tiles);
        if (marks && marks->after_plan && r0 == 0) {
            e = hipEventRecord(marks->after_plan, stream);
            if (e != hipSuccess) return e;
        }
        if (p.bg_kernel)  // the background tiles of a high-spp frame from their streams in HBM
            hipLaunchKernelGGL(background_kernel, dim3(batch_tiles < kQueueGrid ? batch_tiles : kQueueGrid), dim3(kBlock), 0, stream, p.scene, p.ws.tile_draws, out, out8, p, tile_base, batch_tiles);
        const int primary_grid = p.grid_primary > 0 ? p.grid_primary : kPrimaryGrid, resolve_grid = p.grid_resolve > 0 ? p.grid_resolve : kResolveGrid;
        const int pgrid = batch_tiles * p.parts_per_tile < primary_grid ? batch_tiles * p.parts_per_tile : primary_grid;
        with_view(p.scene_in_lds ? (p.scene_posed ? kViewLds : kViewLdsUnposed) : kViewHbm, [&](auto v) {
            constexpr int kView = decltype(v)::value;
            const size_t view_dyn = kView == kViewHbm ? 0 : dyn;
            hipLaunchKernelGGL(primary_kernel<kView>, dim3(pgrid), dim3(kBlock), view_dyn, stream, p, p.scene, draws, out, out8, tile_base, batch_tiles);
            launch_levels<kView>(p, stream, view_dyn, lights);
        });
        const int rgrid = batch_tiles * p.parts_per_tile < resolve_grid ? batch_tiles * p.parts_per_tile : resolve_grid;
        if (p.background == MCRT_BACKGROUND_TRANSPARENT)
            hipLaunchKernelGGL(resolve_transparent_kernel, dim3(rgrid), dim3(kBlock), 0, stream, p, p.scene, out, out8, tile_base);
        else
            hipLaunchKernelGGL(resolve_kernel, dim3(rgrid), dim3(kBlock), 0, stream, p, p.scene, draws, out, out8, tile_base);
        const int batch = r0 / p.rows_per_batch;
        if (marks && batch < marks->n_batch_done) {
            e = hipEventRecord(marks->batch_done[batch], stream);
            if (e != hipSuccess) return e;
        }
    }
    return hipGetLastError();
}

// ---- background and draw plates (kernels.h): q's tile streams seeded in the scratch `tile_rng`, then `kernel` over every tile
template <class Kernel, class Plate>
static hipError_t launch_fill_plate(RenderParams q, Kernel kernel, Plate* plate, uint32_t* tile_rng, hipStream_t stream) {
    q.tile_rng = tile_rng;
    const int n = owned_tiles(q);
    if (n <= 0) return hipErrorInvalidValue;
    hipError_t e = launch_seed_tiles(q, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3((n * q.stream_parts + kStreamWaves - 1) / kStreamWaves), dim3(64 * kStreamWaves), 0, stream, q, plate, n);
    return hipGetLastError();
}
hipError_t launch_fill_bg_plate(const RenderParams& p, float4* plate, uint32_t* tile_rng, hipStream_t stream) {
    if (!bg_plate_eligible(p) || !plate || !tile_rng || bg_plate_bytes(p.cfg) == 0) return hipErrorInvalidValue;
    return launch_fill_plate(bg_plate_fill_params(p), fill_bg_plate_kernel, plate, tile_rng, stream);
}
hipError_t launch_fill_draw_plate(const RenderParams& p, float* plate, uint32_t* tile_rng, hipStream_t stream) {
    if (!draw_plate_eligible(p) || !plate || !tile_rng || draw_plate_bytes(p) == 0) return hipErrorInvalidValue;
    RenderParams q = bg_plate_fill_params(p);
    q.draw_plate = nullptr;
    return launch_fill_plate(q, fill_draw_plate_kernel, plate, tile_rng, stream);
}

// ---- batches ----------------------------------------------------------------------------------
hipError_t launch_seed_tiles_batch(const RenderParams& p0, const RenderParams* d_table, int n_frames, hipStream_t stream) {
    const int n = owned_tiles(p0);
    if (n <= 0 || n_frames <= 0 || p0.draws_per_sample <= 0 || !p0.tile_rng) return hipSuccess;
    const unsigned F = static_cast<unsigned>(n_frames);
    hipLaunchKernelGGL(seed_tiles_batch_kernel, dim3((n + 63) / 64, F), dim3(64), 0, stream, ParamTable(d_table), n);
    if (p0.stream_parts > 1)
        hipLaunchKernelGGL(advance_tiles_batch_kernel, dim3((n + kStreamWaves - 1) / kStreamWaves, F), dim3(64 * kStreamWaves), 0, stream, ParamTable(d_table), n);
    return hipGetLastError();
}

template <int kView>
static void launch_batch_stages(const RenderParams& p0, const BatchPlan& b, const RenderParams* d_table, unsigned F, int n, hipStream_t stream) {
    const int pgrid = n * p0.parts_per_tile < p0.grid_primary ? n * p0.parts_per_tile : p0.grid_primary;
    hipLaunchKernelGGL(primary_batch_kernel<kView>, dim3(pgrid, F), dim3(kBlock), b.dyn, stream, ParamTable(d_table), n);
    if (p0.cfg.ao_enabled && p0.cfg.ao_samples > 0)  // ahead of `lit`, whose last phase applies the AO factor
        hipLaunchKernelGGL(ao_batch_kernel<kView>, dim3(p0.grid_ao, F), dim3(kBlock), b.dyn, stream, ParamTable(d_table));
    hipLaunchKernelGGL(lit_batch_kernel<kView>, dim3(p0.grid_lit, F), dim3(kBlock), b.lit_dyn, stream, ParamTable(d_table));
}

hipError_t launch_render_batch(const RenderParams& p0, const BatchPlan& b, const RenderParams* d_table, int n_frames, hipStream_t stream) {
    const int n = owned_tiles(p0);
    if (n <= 0 || n_frames <= 0) return hipSuccess;
    if (!batch_eligible(p0) || n_frames > kBatchMaxFrames || p0.grid_primary <= 0 || p0.grid_ao <= 0 || p0.grid_lit <= 0 || p0.grid_resolve <= 0)
        return hipErrorInvalidValue;  // (plan_batch sets the grids)
    const unsigned F = static_cast<unsigned>(n_frames);
    const int waves = p0.stream_waves > 0 ? p0.stream_waves : 1;
    hipLaunchKernelGGL(plan_tiles_batch_kernel, dim3((n * waves + kStreamWaves - 1) / kStreamWaves, F), dim3(64 * kStreamWaves), 0, stream, ParamTable(d_table), n);
    if (p0.bg_kernel) hipLaunchKernelGGL(background_batch_kernel, dim3(n < kQueueGrid ? n : kQueueGrid, F), dim3(kBlock), 0, stream, ParamTable(d_table), n);
    with_view(b.view, [&](auto v) { launch_batch_stages<decltype(v)::value>(p0, b, d_table, F, n, stream); });
    const int rgrid = n * p0.parts_per_tile < p0.grid_resolve ? n * p0.parts_per_tile : p0.grid_resolve;
    if (p0.background == MCRT_BACKGROUND_TRANSPARENT)
        hipLaunchKernelGGL(resolve_transparent_batch_kernel, dim3(rgrid, F), dim3(kBlock), 0, stream, ParamTable(d_table));
    else
        hipLaunchKernelGGL(resolve_batch_kernel, dim3(rgrid, F), dim3(kBlock), 0, stream, ParamTable(d_table));
    return hipGetLastError();
}

}  // namespace mcrt
