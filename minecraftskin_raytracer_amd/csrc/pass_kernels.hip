// pass_kernels.hip — the stand-alone passes over a resident scene (not stages of a render): geometry layers and pixel
// picks, the ground shadow, the ground occlusion, the ground reflection, the light layers, the light bake, skin repaints.  They share scene staging and tile geometry with the pipeline (kernel_common.h)
// and nothing else: no workspace, no counters.
#include "kernel_common.h"

// the ground pass's hook (kernel_common.h: verification hooks): tools/ground_class_hooks.h makes the pass write every pixel's
// class (missed, culled by tile, decided, traced) into its visibility plane
#ifndef MCRT_HOOK_GROUND_PIXEL
#define MCRT_HOOK_GROUND_PIXEL(vis, reached, culled, undecided)
#endif

// the ground-occlusion pass's hook: tools/ground_occlusion_class_hooks.h makes the pass write every pixel's class (missed, culled by
// tile, without a candidate, traced) into its occlusion plane
#ifndef MCRT_HOOK_GROUND_OCCLUSION_PIXEL
#define MCRT_HOOK_GROUND_OCCLUSION_PIXEL(occ, reached, culled, traced)
#endif

namespace mcrt {

using namespace rt;

// ---------------------------------------------------------------------------------------------
// geometry layers (kernels.h: LayersFrame): depth, normal, albedo and id planes, and single-pixel picks.  One pixel-centre
// ray per pixel — the reference's primary ray at samplesPerPixel == 1 without depth of field (tile_renderer.cpp:92-103) —
// and intersectScene; no draws, no records, no shading, no workspace.
//   a workgroup per 256 pixels of a screen tile (grid-stride): every wave forms the tile's mesh mask as `plan_tiles` does
//   (tile_mesh_mask without the lens padding); a tile nothing can touch — more than nine in ten of a full-size frame — is
//   filled with the miss constants and builds no ray; the scene tables go to LDS at the workgroup's first touched tile only
//   a touched tile: a lane per pixel, rows of the tile along the lanes, 16 B per lane and plane (the depths of four
//   neighbouring pixels are collected into one lane where the rows are 16-byte aligned)
// ---------------------------------------------------------------------------------------------
struct Surface {  // mcrt_surface in registers
    int mesh, face, tx, ty;
    float t;
    V3 p, n;
    C4 tex;
};
__device__ __forceinline__ Surface miss_surface() {
    return Surface{-1, 0, -1, -1, kFltMax, mk(0.0f, 0.0f, 0.0f), mk(0.0f, 0.0f, 0.0f), C4{0.0f, 0.0f, 0.0f, 0.0f}};
}
// what the pixel-centre ray of (px, py) meets, among the meshes of mesh_mask
template <class SV>
__device__ __forceinline__ Surface pixel_surface(const SV& sc, const mcrt_config& cfg, const float aspect, const int px, const int py,
                                                 const unsigned long long mesh_mask) {
    const float u = (static_cast<float>(px) + 0.5f) / static_cast<float>(cfg.width);
    const float v = (static_cast<float>(py) + 0.5f) / static_cast<float>(cfg.height);
    const Ray ray = camera_ray(sc, u, v, aspect);
    int mesh;
    const Hit h = hit_scene(sc, ray, mesh_mask, &mesh);
    Surface s = miss_surface();
    if (h.hit) {
        s.mesh = mesh;
        s.face = face_slot(h.axis, h.neg) | (h.back ? MCRT_ID_BACK : 0) | (h.outer ? MCRT_ID_OUTER : 0);
        hit_face_texel(sc, mesh, h, s.tx, s.ty);
        s.t = h.t;
        s.p = h.p;
        s.n = h.n;
        s.tex = h.tex;
    }
    return s;
}
// tile_mesh_mask for the pinhole camera: lane m of the calling wave tests mesh m
__device__ __forceinline__ unsigned long long layers_tile_mask(const SceneView& sc, const mcrt_config& cfg, const TileGeom& tg, const float aspect, const int lane) {
    const bool cull = sc.hdr->cull_ok != 0 && sc.n_meshes < 64;
    bool touch = lane < sc.n_meshes;
    if (touch && cull) touch = mesh_touches_tile(sc.meshes[lane], tg, cfg, aspect, 0.0f);
    unsigned long long mask = __ballot(touch);
    if (!cull && sc.n_meshes > 0) mask = ~0ull;
    return mask;
}
// a unit = kBlock pixels of a tile (a touched 32x32 tile is traced by four workgroups, a ray per lane each): the unit's tile,
// and this lane's pixel in it.  Two halves — unit_tile, which is the same in every lane, and lane_pixel — for the reflection
// pass, which forms its mask between them (with the pixel decoded first it takes 16 bytes more scratch); unit_pixel is both.
struct UnitPixel {
    TileGeom tg;
    unsigned p0, npix;  // the unit's first pixel in the tile, the tile's pixels
    bool valid;
    int px, py;
    size_t idx;
};
__device__ __forceinline__ bool unit_tile(const LayersShape& tiles, const int unit, UnitPixel& up) {
    const mcrt_config& cfg = tiles.cfg;
    const int tile = unit / tiles.parts, part = unit - tile * tiles.parts;
    const int tyi = tile / tiles.tiles_x, txi = tile - tyi * tiles.tiles_x;
    TileGeom& tg = up.tg;
    tg.x = txi * cfg.tile_size, tg.y = tyi * cfg.tile_size;
    tg.w = min(cfg.tile_size, cfg.width - tg.x), tg.h = min(cfg.tile_size, cfg.height - tg.y);
    tg.owned_row = tyi, tg.frame_tile = tile;
    up.npix = static_cast<unsigned>(tg.w) * static_cast<unsigned>(tg.h);
    up.p0 = static_cast<unsigned>(part) * kBlock;
    return up.p0 < up.npix;  // a clipped edge tile holds fewer units
}
__device__ __forceinline__ void lane_pixel(const mcrt_config& cfg, const int tid, UnitPixel& up) {
    const TileGeom& tg = up.tg;
    const unsigned pix = up.p0 + static_cast<unsigned>(tid);
    up.valid = pix < up.npix;
    const unsigned uly = UDiv(static_cast<unsigned>(tg.w)).div(up.valid ? pix : 0u);
    up.py = tg.y + static_cast<int>(uly), up.px = tg.x + static_cast<int>((up.valid ? pix : 0u) - uly * static_cast<unsigned>(tg.w));
    up.idx = static_cast<size_t>(up.py) * static_cast<size_t>(cfg.width) + static_cast<size_t>(up.px);
}
__device__ __forceinline__ bool unit_pixel(const LayersShape& tiles, const int unit, const int tid, UnitPixel& up) {
    if (!unit_tile(tiles, unit, up)) return false;
    lane_pixel(tiles.cfg, tid, up);
    return true;
}
// one value per pixel into a plane: 16 bytes per four neighbouring pixels of a row where `quads` (lanes 4k .. 4k+3 then hold
// four neighbours of one row, all valid or none)
__device__ __forceinline__ void store_plane(float* __restrict__ plane, const bool quads, const bool valid, const int lane, const size_t idx, const float val) {
    if (quads) {
        const float v1 = __shfl_down(val, 1), v2 = __shfl_down(val, 2), v3 = __shfl_down(val, 3);
        if (valid && (lane & 3) == 0) *reinterpret_cast<float4*>(plane + idx) = make_float4(val, v1, v2, v3);
    } else if (valid) {
        plane[idx] = val;
    }
}
template <int kView>
__device__ __forceinline__ void layers_body(const LayersFrame& __restrict__ f, const LayersShape& __restrict__ sh) {
    extern __shared__ __align__(16) unsigned char s_dyn[];
    const SceneView scg = view_of(f.scene);
    const mcrt_config& cfg = sh.cfg;
    const int tid = threadIdx.x, lane = tid & 63;
    const float aspect = static_cast<float>(cfg.width) / static_cast<float>(cfg.height);
    // depths as one 16-byte store per four pixels: every tile row starts and ends on a 16-byte boundary of the plane
    const bool quads = (cfg.width & 3) == 0 && (cfg.tile_size & 3) == 0 && (reinterpret_cast<uintptr_t>(f.depth) & 15u) == 0;
    typename ViewSel<kView>::type sc;
    bool staged = false;
    const int n_units = sh.tiles_x * sh.tiles_y * sh.parts;
    for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        UnitPixel up;
        if (!unit_pixel(sh, unit, tid, up)) continue;
        const unsigned long long mask = layers_tile_mask(scg, cfg, up.tg, aspect, lane);  // the same in every wave of the workgroup
        stage_view_once<kView>(scg, f.lds_face_entries, f.lds_alpha_words, s_dyn, mask != 0ull, sc, staged);
        Surface s = miss_surface();
        if (mask != 0ull && up.valid) s = pixel_surface(sc, cfg, aspect, up.px, up.py, mask);
        if (f.depth) store_plane(f.depth, quads, up.valid, lane, up.idx, s.t);
        if (up.valid) {
            if (f.normal) f.normal[up.idx] = make_float4(s.n.x, s.n.y, s.n.z, 0.0f);
            if (f.albedo) f.albedo[up.idx] = make_float4(s.tex.r, s.tex.g, s.tex.b, s.tex.a);
            if (f.id) f.id[up.idx] = make_int4(s.mesh, s.face, s.tx, s.ty);
        }
    }
}
template <int kView>
__global__ __launch_bounds__(kBlock) void layers_kernel(const LayersFrame f, const LayersShape sh) {
    layers_body<kView>(f, sh);
}
using LayersTable = const __attribute__((address_space(4))) LayersFrame*;
template <int kView>
__global__ __launch_bounds__(kBlock) void layers_batch_kernel(LayersTable table, const LayersShape sh) {
    layers_body<kView>(*(const LayersFrame*)(table + blockIdx.y), sh);
}
// a lane per picked pixel, over the HBM view with every mesh tested (the tile masks only leave out meshes that cannot be hit)
__global__ __launch_bounds__(64) void pick_kernel(const uint8_t* __restrict__ scene, const LayersShape sh, const int32_t* __restrict__ xy, const int n,
                                                  mcrt_surface* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const SceneView sc = view_of(scene);
    const float aspect = static_cast<float>(sh.cfg.width) / static_cast<float>(sh.cfg.height);
    const Surface s = pixel_surface(sc, sh.cfg, aspect, xy[2 * i], xy[2 * i + 1], ~0ull);
    float4* o = reinterpret_cast<float4*>(out + i);  // 64 bytes, 16-aligned (hipMalloc)
    o[0] = make_float4(__int_as_float(s.mesh), __int_as_float(s.face), __int_as_float(s.tx), __int_as_float(s.ty));
    o[1] = make_float4(s.t, s.p.x, s.p.y, s.p.z);
    o[2] = make_float4(s.n.x, s.n.y, s.n.z, 0.0f);
    o[3] = make_float4(s.tex.r, s.tex.g, s.tex.b, s.tex.a);
}

// ---------------------------------------------------------------------------------------------
// skins on resident scenes (kernels.h: SkinPaintFrame): a repaintable handle's blob takes a new skin from an RGBA8 image in
// device memory.  One workgroup of 256 threads per scene:
//   the image (16 or 8 KB) and the host's 256 floats u8 / 255.0f go to LDS, 16 bytes per lane where the image's address allows
//   1 lane / pool texel (strides of 256)   its skin pixel through the map, four table reads, one 16-byte store into the pool;
//                                          two ballots per wave — alpha == 0 and alpha > 0, which for a byte is a == 0 and
//                                          a != 0 — interleaved by lanes 0..3 into the wave's four alpha-predicate words;
//                                          a texel with alpha 0 sets its mesh's bit in LDS
//   1 lane / mesh                          the MESH_OPAQUE bit of FlatMesh::flags, an ordinary load and store
// Every store is a vector store; nothing of the blob but the pool, the predicate words and that bit is written.
// ---------------------------------------------------------------------------------------------
constexpr int kSkinBlock = 256;
__device__ __forceinline__ uint32_t spread16(uint32_t x) {  // bit j of the low 16 bits → bit 2j
    x = (x | (x << 8)) & 0x00ff00ffu;
    x = (x | (x << 4)) & 0x0f0f0f0fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}
__device__ __forceinline__ void skin_paint_body(const SkinPaintFrame& __restrict__ f, const SkinPaintShape& __restrict__ sh) {
    __shared__ __align__(16) uint32_t s_skin[64 * 64];
    __shared__ float s_unit[256];
    __shared__ uint32_t s_clear;  // bit m: a texel of mesh m has alpha 0
    const int tid = threadIdx.x, lane = tid & 63;
    const float* __restrict__ unit = static_cast<const float*>(sh.tables);
    const uint16_t* __restrict__ map = reinterpret_cast<const uint16_t*>(unit + 256);
    const int n_pixels = sh.skin_bytes >> 2;
    if ((reinterpret_cast<uintptr_t>(f.skin) & 15u) == 0) {
        const uint4* __restrict__ src = reinterpret_cast<const uint4*>(f.skin);
        for (int i = tid; i < (n_pixels >> 2); i += kSkinBlock) reinterpret_cast<uint4*>(s_skin)[i] = src[i];
    } else {
        const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(f.skin);
        for (int i = tid; i < n_pixels; i += kSkinBlock) s_skin[i] = src[i];
    }
    s_unit[tid] = unit[tid];
    if (tid == 0) s_clear = 0u;
    __syncthreads();
    float4* __restrict__ pool = reinterpret_cast<float4*>(f.scene + sh.texel_offset);
    uint32_t* __restrict__ abits = reinterpret_cast<uint32_t*>(f.scene + sh.alpha_offset);
    for (int base = 0; base < sh.n_texels; base += kSkinBlock) {  // (uniform per workgroup: every wave reaches its ballots)
        const int i = base + tid;
        const bool valid = i < sh.n_texels;
        bool zero = false, positive = false;
        if (valid) {
            const uint32_t entry = map[i];
            const uint32_t px = s_skin[entry & 4095u];
            const uint32_t a = px >> 24;
            pool[i] = make_float4(s_unit[px & 255u], s_unit[(px >> 8) & 255u], s_unit[(px >> 16) & 255u], s_unit[a]);
            zero = a == 0u, positive = a != 0u;
            if (zero) atomicOr(&s_clear, 1u << (entry >> 12));
        }
        const unsigned long long z = __ballot(zero), p = __ballot(positive);
        // the wave's 64 texels are words w0 .. w0 + 3 (a wave starts at a multiple of 64 texels): lane k forms word k
        const uint32_t word = static_cast<uint32_t>(i - lane) / 16u + static_cast<uint32_t>(lane);
        if (lane < 4 && word < sh.alpha_words) {
            const uint32_t zk = static_cast<uint32_t>(z >> (16 * lane)) & 0xffffu, pk = static_cast<uint32_t>(p >> (16 * lane)) & 0xffffu;
            abits[word] = spread16(zk) | (spread16(pk) << 1);
        }
    }
    __syncthreads();
    if (tid < sh.n_meshes) {
        FlatMesh* fm = reinterpret_cast<FlatMesh*>(f.scene + sh.mesh_offset) + tid;
        const uint32_t flags = fm->flags;
        fm->flags = ((s_clear >> tid) & 1u) ? (flags & ~MESH_OPAQUE) : (flags | MESH_OPAQUE);
    }
}
__global__ __launch_bounds__(kSkinBlock) void skin_paint_kernel(const SkinPaintFrame f, const SkinPaintShape sh) { skin_paint_body(f, sh); }
using SkinPaintTable = const __attribute__((address_space(4))) SkinPaintFrame*;
__global__ __launch_bounds__(kSkinBlock) void skin_paint_batch_kernel(SkinPaintTable table, const SkinPaintShape sh) {  // a batch of one kind
    skin_paint_body(*(const SkinPaintFrame*)(table + blockIdx.y), sh);
}
// A batch may mix the two 64x64 models (classic, slim): their tables, texel counts and alpha words differ, so both shapes
// travel by value and a workgroup takes the one its frame names.  `kind` comes from the frame table through blockIdx.y and the
// shapes from the kernel arguments — all uniform, scalar loads and scalar selects — so the texel loop's bound and the
// `word < alpha_words` guard stay wave-uniform and every wave reaches both ballots.
__global__ __launch_bounds__(kSkinBlock) void skin_paint_mixed_kernel(SkinPaintTable table, const SkinPaintShape sh0, const SkinPaintShape sh1) {
    const SkinPaintFrame f = *(const SkinPaintFrame*)(table + blockIdx.y);
    const bool second = f.kind != 0;
    SkinPaintShape sh;
    sh.tables = second ? sh1.tables : sh0.tables;
    sh.n_texels = second ? sh1.n_texels : sh0.n_texels;
    sh.n_meshes = second ? sh1.n_meshes : sh0.n_meshes;
    sh.skin_bytes = second ? sh1.skin_bytes : sh0.skin_bytes;
    sh.mesh_offset = second ? sh1.mesh_offset : sh0.mesh_offset;
    sh.texel_offset = second ? sh1.texel_offset : sh0.texel_offset;
    sh.alpha_offset = second ? sh1.alpha_offset : sh0.alpha_offset;
    sh.alpha_words = second ? sh1.alpha_words : sh0.alpha_words;
    skin_paint_body(f, sh);
}

// ---------------------------------------------------------------------------------------------
// capes on resident scenes (kernels.h: CapePaintFrame): a caped handle's blob takes a new cape from a 64x32 RGBA8 image in
// device memory (NULL: a transparent one).  One workgroup of 256 threads per scene:
//   the host's 256 floats u8 / 255.0f go to LDS — four reads per texel at indices the image decides
//   1 lane / pool texel (372: two strides of 256)   its cape pixel through the map, four table reads, one 16-byte store; the
//                                                    two ballots per wave and their interleaving as in skin_paint_body;
//                                                    lanes past texel 371 contribute zero bits, as the flattener leaves them
//   lane 0                                           the cape mesh's MESH_OPAQUE bit, an ordinary load and store
// The IMAGE is not staged in LDS.  The unwrap reads 88 bytes of each of 17 rows, every pixel once: 17 cache lines of 128 bytes
// in all, seven or so per wave load (a face is 10 texels wide), each fetched once — staging would put a second barrier and an
// LDS round trip behind the same 17 line fetches and buy no reuse.  The skin kernel stages because its image is read whole,
// 16 bytes per lane; here a third of 17 rows is read, 4 bytes per lane.
// Every store is a vector store; nothing of the blob but the cape's 372 texels, its 24 predicate words and that bit is written.
// ---------------------------------------------------------------------------------------------
constexpr int kCapeBlock = 256;
static_assert(kCapeAlphaWords == (kCapeTexels + 15) / 16, "cape_paint_body: the cape's alpha-predicate words");
__device__ __forceinline__ void cape_paint_body(const CapePaintFrame& __restrict__ f, const CapePaintShape& __restrict__ sh) {
    __shared__ float s_unit[256];
    const int tid = threadIdx.x, lane = tid & 63;
    const float* __restrict__ unit = static_cast<const float*>(sh.tables);
    const uint16_t* __restrict__ map = reinterpret_cast<const uint16_t*>(unit + 256);
    s_unit[tid] = unit[tid];
    __syncthreads();
    const uint32_t* __restrict__ cape = reinterpret_cast<const uint32_t*>(f.cape);
    float4* __restrict__ pool = reinterpret_cast<float4*>(f.scene + f.texel_offset);
    uint32_t* __restrict__ abits = reinterpret_cast<uint32_t*>(f.scene + f.alpha_offset);
    bool any_zero = false;
    for (int base = 0; base < kCapeTexels; base += kCapeBlock) {  // (uniform per workgroup: every wave reaches its ballots)
        const int i = base + tid;
        bool zero = false, positive = false;
        if (i < kCapeTexels) {
            const uint32_t px = cape ? cape[map[i]] : 0u;  // (`cape` is uniform)
            const uint32_t a = px >> 24;
            pool[i] = make_float4(s_unit[px & 255u], s_unit[(px >> 8) & 255u], s_unit[(px >> 16) & 255u], s_unit[a]);
            zero = a == 0u, positive = a != 0u;
            any_zero = any_zero || zero;
        }
        const unsigned long long z = __ballot(zero), p = __ballot(positive);
        // the wave's 64 texels are words w0 .. w0 + 3 (a wave starts at a multiple of 64 texels): lane k forms word k
        const uint32_t word = static_cast<uint32_t>(i - lane) / 16u + static_cast<uint32_t>(lane);
        if (lane < 4 && word < static_cast<uint32_t>(kCapeAlphaWords)) {
            const uint32_t zk = static_cast<uint32_t>(z >> (16 * lane)) & 0xffffu, pk = static_cast<uint32_t>(p >> (16 * lane)) & 0xffffu;
            abits[word] = spread16(zk) | (spread16(pk) << 1);
        }
    }
    const int clear = __syncthreads_or(any_zero ? 1 : 0);
    if (tid == 0) {
        uint32_t* flags = reinterpret_cast<uint32_t*>(f.scene + f.flags_offset);
        const uint32_t current = *flags;
        *flags = clear ? (current & ~static_cast<uint32_t>(MESH_OPAQUE)) : (current | MESH_OPAQUE);
    }
}
__global__ __launch_bounds__(kCapeBlock) void cape_paint_kernel(const CapePaintFrame f, const CapePaintShape sh) { cape_paint_body(f, sh); }
using CapePaintTable = const __attribute__((address_space(4))) CapePaintFrame*;
__global__ __launch_bounds__(kCapeBlock) void cape_paint_batch_kernel(CapePaintTable table, const CapePaintShape sh) {
    cape_paint_body(*(const CapePaintFrame*)(table + blockIdx.y), sh);
}

// ---------------------------------------------------------------------------------------------
// views of resident scenes (kernels.h: SceneViewFrame): a repaintable handle's blob takes the header and the mesh table of
// another pose, camera and light from a table the host flattened.  One wave per scene:
//   lane i   chunks i, i + 64, i + 128 of the prefix [0, texel_offset), 16 bytes each, one load and one store per chunk;
//            the chunk that holds a mesh's `flags` (byte 68 of its FlatMesh: word 1 of the chunk at byte 64) first loads the
//            blob's own word and keeps its MESH_OPAQUE bit — the skin's, not the view's
// A lane reads and writes its own chunks only: no LDS, no barrier.  Every store is a vector store; nothing from texel_offset
// on is written.
// ---------------------------------------------------------------------------------------------
constexpr int kViewBlock = 64;
constexpr uint32_t kMeshChunks = sizeof(FlatMesh) / 16, kFlagsChunk = 4;  // chunks per mesh; the one with `flags`, as word 1
static_assert(sizeof(FlatMesh) % 16 == 0 && offsetof(FlatMesh, flags) == kFlagsChunk * 16 + 4, "scene_view_body: where FlatMesh::flags lies");
static_assert(kViewMaxChunks == 3 * kViewBlock, "scene_view_body: three chunks per lane");
__device__ __forceinline__ void scene_view_body(const SceneViewFrame& __restrict__ f, const SceneViewShape& __restrict__ sh) {
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(f.table);
    uint4* dst = reinterpret_cast<uint4*>(f.scene);
    const uint32_t first = sh.mesh_offset / 16u + kFlagsChunk;  // mesh 0's flags chunk
    const uint32_t n_chunks = static_cast<uint32_t>(sh.n_chunks);
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
        const uint32_t c = threadIdx.x + k * kViewBlock;
        if (c >= n_chunks) break;
        uint4 v = src[c];
        const uint32_t r = c - first;
        if (c >= first && r % kMeshChunks == 0u && r / kMeshChunks < static_cast<uint32_t>(sh.n_meshes)) {
            const uint32_t current = reinterpret_cast<const uint32_t*>(f.scene)[4u * c + 1u];
            v.y = (v.y & ~static_cast<uint32_t>(MESH_OPAQUE)) | (current & MESH_OPAQUE);
        }
        dst[c] = v;
    }
}
__global__ __launch_bounds__(kViewBlock) void scene_view_kernel(const SceneViewFrame f, const SceneViewShape sh) { scene_view_body(f, sh); }
using SceneViewTable = const __attribute__((address_space(4))) SceneViewFrame*;
__global__ __launch_bounds__(kViewBlock) void scene_view_batch_kernel(SceneViewTable table, const SceneViewShape sh) {
    scene_view_body(*(const SceneViewFrame*)(table + blockIdx.y), sh);
}

// ---------------------------------------------------------------------------------------------
// ground shadow (kernels.h: GroundFrame): the figure's soft shadow on the plane y = ground_y, as planes of their own.  Per
// pixel the layers' pixel-centre ray, its point P on the plane, and computeSoftShadow(P, (0, 1, 0)) (shading.cpp:28-60) with
// the seed of a hit at depth 0 (raytracer.cpp:110-112) — the figure in front of the plane plays no part.  No workspace.
//   a workgroup per 256 pixels of a screen tile (grid-stride), in the phases of `lit`, handed over through LDS:
//   1 lane / mesh (every wave)   which meshes can shadow ANY ground point under the tile (ground_tile_mask): none for most
//                                tiles of a frame — their reached pixels are fully lit without a classification or a ray
//   1 lane / pixel               ray, plane hit, P; the whole-bundle decision (rt::bundle_classify) from P + N * 1e-3f: lit by
//                                all S light samples, by none, or undecided with a candidate mask; the undecided are packed
//   1 lane / undecided pixel     truncated mt19937 (mt[397] from the seed table) → 2·S draws → S disk sample positions in LDS
//   1 lane / (undecided pixel, light sample)   exact any-hit test on the candidates → lit count by ballot
//                                (these three phases: resolve_shadow_bundles, kernel_common.h)
//   1 lane / pixel               visibility = lit / S, distance, matte: coalesced stores, 16 bytes per four pixels of a row
//                                where the rows allow
// ---------------------------------------------------------------------------------------------
constexpr int kGroundWaves = 4;  // waves per SIMD the kernels are built for: `lit`'s, whose device functions they inline
struct GroundPoint {
    bool reached;
    float t;  // FLT_MAX where the ray does not reach the plane
    V3 P;
};
// the ray through (fx, fy) pixels of the frame — a pixel centre is (px + 0.5f, py + 0.5f) — against the plane y = g
__device__ __forceinline__ GroundPoint ground_point(const SceneView& sc, const mcrt_config& cfg, const float aspect, const float g, const float fx,
                                                    const float fy) {
    const float u = fx / static_cast<float>(cfg.width);
    const float v = fy / static_cast<float>(cfg.height);
    const Ray ray = camera_ray(sc, u, v, aspect);
    const float t = (g - ray.o.y) / ray.d.y;
    GroundPoint h;
    h.reached = ray.d.y != 0.0f && t > 0.0f && t <= kFltMax;
    h.t = h.reached ? t : kFltMax;
    h.P = mk(ray.o.x + ray.d.x * t, g, ray.o.z + ray.d.z * t);
    return h;
}
// The tile's footprint on the plane y = g: the bounding rectangle of the points where its four corner rays meet the plane,
// and `reach`, the largest of their distances along x, z and the ray.  ok: all four reach the plane well away from the
// horizon (|d.y| >= 1e-2) at finite points; otherwise the callers keep every mesh.
struct TileFootprint {
    bool ok;
    float x0, x1, z0, z1, reach;
};
__device__ __forceinline__ TileFootprint tile_footprint(const SceneView& sc, const mcrt_config& cfg, const TileGeom& tg, const float aspect, const float g) {
    TileFootprint fp{true, kFltMax, -kFltMax, kFltMax, -kFltMax, 0.0f};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float fx = static_cast<float>(tg.x + ((c & 1) ? tg.w : 0)), fy = static_cast<float>(tg.y + ((c & 2) ? tg.h : 0));
        const Ray ray = camera_ray(sc, fx / static_cast<float>(cfg.width), fy / static_cast<float>(cfg.height), aspect);
        const float t = (g - ray.o.y) / ray.d.y;
        fp.ok = fp.ok && __builtin_fabsf(ray.d.y) >= 1e-2f && t > 0.0f && t < 1e30f;
        const float dx = ray.d.x * t, dz = ray.d.z * t;
        const float x = ray.o.x + dx, z = ray.o.z + dz;
        fp.x0 = __builtin_fminf(fp.x0, x), fp.x1 = __builtin_fmaxf(fp.x1, x), fp.z0 = __builtin_fminf(fp.z0, z), fp.z1 = __builtin_fmaxf(fp.z1, z);
        fp.reach = __builtin_fmaxf(fp.reach, __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(dx), __builtin_fabsf(dz)), t));
        fp.ok = fp.ok && x == x && z == z;  // (fmin / fmax drop a NaN)
    }
    return fp;
}
// world bounds of a mesh: its box, or its padded bounding sphere's when it is posed; false for a sphere without a radius
__device__ __forceinline__ bool mesh_world_bounds(const FlatMesh& m, V3& lo, V3& hi) {
    lo = ld3(m.lo), hi = ld3(m.hi);
    if (!(m.flags & MESH_ROTATED)) return true;
    const float r = m.sphere[3];
    lo = mk(m.sphere[0] - r, m.sphere[1] - r, m.sphere[2] - r);
    hi = mk(m.sphere[0] + r, m.sphere[1] + r, m.sphere[2] + r);
    return r >= 0.0f;
}
// The meshes that can shadow a ground point under the tile, conservatively: lane m of the calling wave tests mesh m.
// The tile's pixel-centre rays lie inside its four corner rays; when all four reach the plane (well away from the horizon:
// |d.y| >= 1e-2) the ground points of the tile lie in the bounding rectangle F of the four corner points — the image of a
// screen rectangle on a plane in front of the camera is a convex quadrilateral.  A shadow ray leaves Q + (0, 1e-3, 0) for a
// target T within Rb of the light centre L.  When the lowest target is above the top of a mesh's world box B (bounding
// sphere when posed) and above the origins, the ray climbs, and it meets B at a point X with gy <= X.y <= B.hi.y only if
// Q = X + (X - T) * k', 0 <= k' <= k = (L.y - Rb - gy) / (L.y - Rb - B.hi.y) - 1: per axis Q lies in
// [B.lo - max(0, L + Rb - B.lo) * k, B.hi + max(0, B.hi - L + Rb) * k] — B's shadow from the light centre, widened by the
// light's radius in the ratio of B's height to the light's clearance.  A mesh whose interval misses F on x or z, with margins
// far above the float error of the points (2e-3 of the footprint's reach, 1e-4 of the interval, 16 slacks), shadows no
// pixel of the tile.  Every other case keeps the mesh: a light that is not clear above the box, a corner that misses the
// plane or grazes it, 64 meshes or more, cull_ok == 0, non-finite values (every comparison is written to fail open).
__device__ __forceinline__ unsigned long long ground_tile_mask(const SceneView& sc, const mcrt_config& cfg, const TileGeom& tg, const float aspect,
                                                               const float g, const float R, const int lane) {
    const int n = sc.n_meshes;
    if (n <= 0) return 0ull;
    const unsigned long long all = n < 64 ? (1ull << n) - 1ull : ~0ull;
    if (sc.hdr->cull_ok == 0 || n >= 64) return all;
    const float slack = sc.hdr->mask_slack;
    const TileFootprint fp = tile_footprint(sc, cfg, tg, aspect, g);
    const float fx0 = fp.x0, fx1 = fp.x1, fz0 = fp.z0, fz1 = fp.z1;
    if (!(fp.ok && fp.reach < 1e30f && slack < 1e30f)) return all;
    const float fm = 2e-3f * fp.reach + 16.0f * slack;
    const V3 L = ld3(sc.hdr->light_pos);
    const float Rb = R * 1.001f + slack;
    const float gy = g + 1e-3f;     // the shadow rays' origins
    const float low = L.y - Rb;     // the lowest target
    bool touch = lane < n;
    if (touch) {
        const FlatMesh& m = sc.meshes[lane];
        if (m.flags & MESH_EMPTY) {
            touch = false;  // intersection.cpp:205: never hit
        } else {
            V3 lo, hi;
            const bool bounded = mesh_world_bounds(m, lo, hi);
            const float h = low - gy, c = low - hi.y;  // the light's height above the origins and above the box
            if (bounded && h > 0.0f && c > 0.01f * h && c > 64.0f * slack) {
                if (hi.y < gy - 64.0f * slack) {
                    touch = false;  // the box ends below the origins and every ray climbs
                } else {
                    const float k = __builtin_fmaxf(h / c - 1.0f, 0.0f);
                    const float qx0 = lo.x - __builtin_fmaxf(0.0f, L.x + Rb - lo.x) * k, qx1 = hi.x + __builtin_fmaxf(0.0f, hi.x - L.x + Rb) * k;
                    const float qz0 = lo.z - __builtin_fmaxf(0.0f, L.z + Rb - lo.z) * k, qz1 = hi.z + __builtin_fmaxf(0.0f, hi.z - L.z + Rb) * k;
                    const float mg = fm + 1e-4f * (__builtin_fabsf(qx0) + __builtin_fabsf(qx1) + __builtin_fabsf(qz0) + __builtin_fabsf(qz1));
                    const bool out = (qx1 + mg < fx0) | (qx0 - mg > fx1) | (qz1 + mg < fz0) | (qz0 - mg > fz1);
                    touch = !out;
                }
            }
        }
    }
    return __ballot(touch);
}
// the 8-bit matte of a value per pixel, (u8)(clamp(1 - val, 0, 1) * 255 + 0.5): four pixels of a row per word where `quads`
// (as store_plane)
__device__ __forceinline__ void store_matte(uint8_t* __restrict__ matte, const bool quads, const bool valid, const int lane, const size_t idx, const float val) {
    const uint32_t a = static_cast<unsigned char>(sclamp(1.0f - val, 0.0f, 1.0f) * 255.0f + 0.5f);
    if (quads) {
        const uint32_t a1 = __shfl_down(a, 1), a2 = __shfl_down(a, 2), a3 = __shfl_down(a, 3);
        if (valid && (lane & 3) == 0) *reinterpret_cast<uint32_t*>(matte + idx) = a | (a1 << 8) | (a2 << 16) | (a3 << 24);
    } else if (valid) {
        matte[idx] = static_cast<uint8_t>(a);
    }
}
template <int kView>
__device__ __forceinline__ void ground_body(const GroundFrame& __restrict__ f, const GroundShape& __restrict__ sh) {
    extern __shared__ __align__(16) unsigned char s_dyn[];  // [scene tables][GroundArea][positions: pass x S x 3 floats]
    __shared__ int s_wcnt[kBlock / 64];
    const SceneView scg = view_of(f.scene);
    const mcrt_config& cfg = sh.tiles.cfg;
    const int tid = threadIdx.x, lane = tid & 63;
    const float aspect = static_cast<float>(cfg.width) / static_cast<float>(cfg.height);
    const float g = f.ground_y;
    const V3 N = mk(0.0f, 1.0f, 0.0f);
    constexpr bool kPosed = kView != kViewLdsUnposed;
    GroundArea& area = *reinterpret_cast<GroundArea*>(s_dyn + scene_tables_lds_span(f.lds_face_entries, f.lds_alpha_words));
    const ShadowBundles sb = shadow_bundles(header_light(scg), sh.samples, sh.pass, sh.bundle_decisions, sh.inside_fast, f.seed_table, area.cand, area.ins, area.count,
                                            area.list, reinterpret_cast<float*>(&area + 1), s_wcnt);
    // four neighbouring pixels of a row per store: every tile row starts and ends on a four-pixel boundary of the plane
    const bool quad_rows = (cfg.width & 3) == 0 && (cfg.tile_size & 3) == 0;
    const bool quads_vis = quad_rows && (reinterpret_cast<uintptr_t>(f.visibility) & 15u) == 0;
    const bool quads_dist = quad_rows && (reinterpret_cast<uintptr_t>(f.distance) & 15u) == 0;
    const bool quads_matte = quad_rows && (reinterpret_cast<uintptr_t>(f.matte) & 3u) == 0;
    typename ViewSel<kView>::type sc;
    bool staged = false;
    const int n_units = sh.tiles.tiles_x * sh.tiles.tiles_y * sh.tiles.parts;
    for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        UnitPixel up;
        if (!unit_pixel(sh.tiles, unit, tid, up)) continue;
        const unsigned long long mask = ground_tile_mask(scg, cfg, up.tg, aspect, g, sb.R, lane);  // the same in every wave of the workgroup
        stage_view_once<kView>(scg, f.lds_face_entries, f.lds_alpha_words, s_dyn, mask != 0ull, sc, staged);
        GroundPoint gp = ground_point(scg, cfg, aspect, g, static_cast<float>(up.px) + 0.5f, static_cast<float>(up.py) + 0.5f);
        if (!up.valid) gp.reached = false, gp.t = kFltMax;
        if (f.distance) store_plane(f.distance, quads_dist, up.valid, lane, up.idx, gp.t);
        uint32_t lit = sb.pairs;  // a pixel that misses the plane, and every pixel of a tile no mesh can shadow
        [[maybe_unused]] bool undecided = false;  // (the hook's)
        if (mask != 0ull) {  // uniform
            // ---- resolve_shadow_bundles: the pixel's point goes to LDS as P.x, P.z; the normal is the plane's
            if (gp.reached) area.pxz[tid] = make_float2(gp.P.x, gp.P.z);
            undecided = resolve_shadow_bundles<kPosed>(scg, sc, sb, header_light(scg), gp.reached, gp.P + N * 1e-3f, mask, 0,
                                                       [&](const uint32_t k, V3& P, V3& Nk) __attribute__((always_inline)) {
                                                           const float2 xz = area.pxz[k];
                                                           P = mk(xz.x, g, xz.y), Nk = N;
                                                       },
                                                       lit);
            // (behind the resolver nothing of the unit is read across lanes any more, so the next unit may overwrite the area)
        }
        // ---- a lane per pixel: the planes
        float vis = static_cast<float>(lit) / static_cast<float>(sb.pairs);
        MCRT_HOOK_GROUND_PIXEL(vis, gp.reached, mask == 0ull, undecided)
        if (f.visibility) store_plane(f.visibility, quads_vis, up.valid, lane, up.idx, vis);
        if (f.matte) store_matte(f.matte, quads_matte, up.valid, lane, up.idx, vis);
    }
}
template <int kView>
__global__ __launch_bounds__(kBlock, kGroundWaves) void ground_kernel(const GroundFrame f, const GroundShape sh) {
    ground_body<kView>(f, sh);
}
using GroundTable = const __attribute__((address_space(4))) GroundFrame*;
template <int kView>
__global__ __launch_bounds__(kBlock, kGroundWaves) void ground_batch_kernel(GroundTable table, const GroundShape sh) {
    ground_body<kView>(*(const GroundFrame*)(table + blockIdx.y), sh);
}

// ---------------------------------------------------------------------------------------------
// ground occlusion (kernels.h: GroundOcclusionFrame): the figure's contact occlusion on the plane y = ground_y, as planes of their
// own.  Per pixel the ground pass's ray and point P, and computeAO(P, (0, 1, 0)) (raytracer.cpp:38-78) with the seed of a hit at P
// (raytracer.cpp:122-123).  No workspace.  Only the pixels within ao_radius of a box are traced — a few per cent of a frame — so
// the rays, not the pixels, are spread over the lanes:
//   a workgroup per 256 pixels of a screen tile (grid-stride), in the phases of the ground pass, handed over through LDS:
//   1 lane / mesh (every wave)   which meshes an AO ray from ANY ground point under the tile can meet (ground_occlusion_tile_mask):
//                                none for most tiles of a frame — their pixels are unoccluded without a point or a ray
//   1 lane / pixel               ray, plane hit, P; the meshes a ray of its hemisphere can meet within the radius
//                                (rt::hemisphere_candidates) among the tile's; the pixels with one are packed
//   1 lane / traced pixel        truncated mt19937 (mt[397] from the table of all seeds where the handle has it) → 2·A draws → the
//                                A world directions in LDS (AoStream)
//   1 lane / (traced pixel, sample)   exact any-hit test within the radius on the candidates → occluded count by ballot
//                                (count_item_rays)
//   1 lane / pixel               occlusion = 1 - occluded / A, matte: coalesced stores, 16 bytes per four pixels of a row where
//                                the rows allow
// ---------------------------------------------------------------------------------------------
// The meshes an AO ray of the tile can meet, conservatively: lane m of the calling wave tests mesh m.  The ground points of the
// tile lie in the bounding rectangle F of its four corner points, as for ground_tile_mask.  A ray leaves O = Q + (0, 1e-3, 0),
// never downwards (its y component is sqrt(r1) >= 0 before and after the normalisation), and is cut at `radius`: it meets a
// mesh's world box B (bounding sphere when posed) only at a point within radius of O and not below it.  So Q lies within
// Rr = radius * 1.001 + slack of B on x and z, B reaches up to the origins' height gy = g + 1e-3 and starts below gy + Rr.  A
// mesh that misses one of these, with margins far above the float error of the points (2e-3 of the footprint's reach, 16
// slacks; 64 slacks and 1e-5 of the heights on y), occludes no pixel of the tile.  Every other case keeps the mesh: a corner
// that misses the plane or grazes it, 64 meshes or more, cull_ok == 0, a negative sphere radius, non-finite values (every
// comparison is written to fail open).
__device__ __forceinline__ unsigned long long ground_occlusion_tile_mask(const SceneView& sc, const mcrt_config& cfg, const TileGeom& tg, const float aspect,
                                                                         const float g, const float radius, const int lane) {
    const int n = sc.n_meshes;
    if (n <= 0) return 0ull;
    const unsigned long long all = n < 64 ? (1ull << n) - 1ull : ~0ull;
    if (sc.hdr->cull_ok == 0 || n >= 64) return all;
    const float slack = sc.hdr->mask_slack;
    const TileFootprint fp = tile_footprint(sc, cfg, tg, aspect, g);
    const float fx0 = fp.x0, fx1 = fp.x1, fz0 = fp.z0, fz1 = fp.z1;
    const float Rr = radius * 1.001f + slack;
    if (!(fp.ok && fp.reach < 1e30f && slack < 1e30f && Rr < 1e30f)) return all;
    const float fm = 2e-3f * fp.reach + 16.0f * slack;
    const float gy = g + 1e-3f;  // the AO rays' origins
    bool touch = lane < n;
    if (touch) {
        const FlatMesh& m = sc.meshes[lane];
        if (m.flags & MESH_EMPTY) {
            touch = false;  // intersection.cpp:205: never hit
        } else {
            V3 lo, hi;
            if (mesh_world_bounds(m, lo, hi)) {
                const float mx = fm + 1e-4f * (__builtin_fabsf(lo.x) + __builtin_fabsf(hi.x) + __builtin_fabsf(lo.z) + __builtin_fabsf(hi.z));
                const float my = 64.0f * slack + 1e-5f * (__builtin_fabsf(gy) + __builtin_fabsf(lo.y) + __builtin_fabsf(hi.y));
                const bool out = (hi.y < gy - my) | (lo.y > gy + Rr + my) | (hi.x + Rr + mx < fx0) | (lo.x - Rr - mx > fx1) | (hi.z + Rr + mx < fz0) |
                                 (lo.z - Rr - mx > fz1);
                touch = !out;
            }
        }
    }
    return __ballot(touch);
}
template <int kView>
__device__ __forceinline__ void ground_occlusion_body(const GroundOcclusionFrame& __restrict__ f, const GroundOcclusionShape& __restrict__ sh) {
    extern __shared__ __align__(16) unsigned char s_dyn[];  // [scene tables][GroundArea][directions: pass x A x 3 floats]
    __shared__ int s_wcnt[kBlock / 64];
    const SceneView scg = view_of(f.scene);
    const mcrt_config& cfg = sh.tiles.cfg;
    const int tid = threadIdx.x, lane = tid & 63;
    const float aspect = static_cast<float>(cfg.width) / static_cast<float>(cfg.height);
    const float g = f.ground_y;
    const int A = sh.ao_samples;
    const float radius = sh.ao_radius;
    const bool live = radius > 0.0f;  // otherwise no ray can be occluded
    const uint32_t rays = static_cast<uint32_t>(A);  // rays per traced pixel
    const uint32_t pass = static_cast<uint32_t>(sh.pass);
    const V3 N = mk(0.0f, 1.0f, 0.0f);
    constexpr bool kPosed = kView != kViewLdsUnposed;
    GroundArea& area = *reinterpret_cast<GroundArea*>(s_dyn + scene_tables_lds_span(f.lds_face_entries, f.lds_alpha_words));
    float* s_dir = reinterpret_cast<float*>(&area + 1);
    // four neighbouring pixels of a row per store: every tile row starts and ends on a four-pixel boundary of the plane
    const bool quad_rows = (cfg.width & 3) == 0 && (cfg.tile_size & 3) == 0;
    const bool quads_occ = quad_rows && (reinterpret_cast<uintptr_t>(f.occlusion) & 15u) == 0;
    const bool quads_matte = quad_rows && (reinterpret_cast<uintptr_t>(f.matte) & 3u) == 0;
    typename ViewSel<kView>::type sc;
    bool staged = false;
    const int n_units = sh.tiles.tiles_x * sh.tiles.tiles_y * sh.tiles.parts;
    for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        UnitPixel up;
        if (!unit_pixel(sh.tiles, unit, tid, up)) continue;
        const unsigned long long mask = live ? ground_occlusion_tile_mask(scg, cfg, up.tg, aspect, g, radius, lane) : 0ull;  // the same in every wave of the workgroup
        stage_view_once<kView>(scg, f.lds_face_entries, f.lds_alpha_words, s_dyn, mask != 0ull, sc, staged);
        uint32_t occluded = 0u;  // a pixel that misses the plane or has no candidate, and every pixel of a tile no mesh can occlude
        bool traced = false;
#ifdef MCRT_KERNEL_HOOKS
        const bool reached = up.valid && ground_point(scg, cfg, aspect, g, static_cast<float>(up.px) + 0.5f, static_cast<float>(up.py) + 0.5f).reached;
#endif
        if (mask != 0ull) {  // uniform
            // ---- a lane per pixel: the plane point and the meshes its hemisphere can meet
            if (up.valid) {
                const GroundPoint gp = ground_point(scg, cfg, aspect, g, static_cast<float>(up.px) + 0.5f, static_cast<float>(up.py) + 0.5f);
                if (gp.reached) {
                    const V3 O = gp.P + N * 1e-3f;
                    const unsigned long long cand = hemisphere_candidates<kPosed>(scg, O, N, radius) & mask;
                    traced = cand != 0ull || scg.n_meshes > 64;  // meshes beyond the mask are tested per ray
                    if (traced) {
                        area.cand[tid] = cand;
                        area.ins[tid] = sh.inside_fast ? origin_inside_boxes(sc, O, cand) : 0ull;  // every ray of the pixel starts there
                        area.pxz[tid] = make_float2(gp.P.x, gp.P.z);
                    }
                }
            }
            area.count[tid] = 0u;
            int total = 0;
            const int rank = block_rank(traced, s_wcnt, total);
            if (traced) area.list[rank] = static_cast<uint32_t>(tid);
            const uint32_t n_traced = static_cast<uint32_t>(total);
            if (n_traced) __syncthreads();  // uniform
            for (uint32_t u0 = 0; u0 < n_traced; u0 += pass) {  // uniform
                const uint32_t nu = min(pass, n_traced - u0);
                if (u0) __syncthreads();  // the previous pass's rays have read the directions
                // ---- a lane per traced pixel: its AoStream, the A directions into LDS
                if (static_cast<uint32_t>(tid) < nu) {
                    const float2 xz = area.pxz[area.list[u0 + tid]];
                    float* dst = s_dir + static_cast<size_t>(tid) * 3 * rays;
                    AoStream ao(f.seed_table_full, mk(xz.x, g, xz.y), N);
                    for (int i = 0; i < A; ++i) {
                        const V3 world = ao.next();
                        dst[3 * i + 0] = world.x;
                        dst[3 * i + 1] = world.y;
                        dst[3 * i + 2] = world.z;
                    }
                }
                __syncthreads();
                // ---- a lane per (traced pixel, sample): count_item_rays over the any-hit test within the radius
                count_item_rays(area.list + u0, nu, rays, area.count, [&](const uint32_t k, const uint32_t q) __attribute__((always_inline)) {
                    const float2 xz = area.pxz[k];
                    const V3 O = mk(xz.x, g, xz.y) + N * 1e-3f;
                    return any_hit_masked(sc, Ray{O, ld3(s_dir + static_cast<size_t>(q) * 3)}, radius, area.cand[k], area.ins[k]);
                });
            }
            // the counts are complete; behind this barrier nothing of the unit is read across lanes any more, so the next
            // unit may overwrite the area
            if (n_traced) __syncthreads();
            if (traced) occluded = area.count[tid];
        }
        // ---- a lane per pixel: the planes
        float occ = 1.0f - static_cast<float>(occluded) / static_cast<float>(A);  // raytracer.cpp:77
        MCRT_HOOK_GROUND_OCCLUSION_PIXEL(occ, reached, mask == 0ull, traced)
        if (f.occlusion) store_plane(f.occlusion, quads_occ, up.valid, lane, up.idx, occ);
        if (f.matte) store_matte(f.matte, quads_matte, up.valid, lane, up.idx, occ);
    }
}
template <int kView>
__global__ __launch_bounds__(kBlock, kGroundWaves) void ground_occlusion_kernel(const GroundOcclusionFrame f, const GroundOcclusionShape sh) {
    ground_occlusion_body<kView>(f, sh);
}
using GroundOcclusionTable = const __attribute__((address_space(4))) GroundOcclusionFrame*;
template <int kView>
__global__ __launch_bounds__(kBlock, kGroundWaves) void ground_occlusion_batch_kernel(GroundOcclusionTable table, const GroundOcclusionShape sh) {
    ground_occlusion_body<kView>(*(const GroundOcclusionFrame*)(table + blockIdx.y), sh);
}

// ---------------------------------------------------------------------------------------------
// ground reflection (kernels.h: ReflectionFrame): the figure mirrored in the plane y = ground_y, as planes of their own.  Per
// pixel the layers' pixel-centre ray, its point P on the plane, the reference's reflection ray for a hit at P with normal
// (0, 1, 0) (raytracer.cpp:134-140) and traceRay(that ray, depth 1) (raytracer.cpp:82-148): the colour the recursion would
// return for a floor at depth 0.  No ambient occlusion (depth 0 only), a bounced miss folds the flat background.  No workspace.
//   a workgroup per 256 pixels of a screen tile (grid-stride), in phases handed over through LDS:
//   1 lane / mesh (every wave)   which meshes a reflection ray of the tile can meet (reflection_tile_mask): none for most
//                                tiles of a frame — they get the miss constants and form no ray
//   1 lane / pixel               ray, plane point, reflection ray, closest hit among the tile's meshes; the hits are packed
//                                onto the block's first lanes as records in LDS (point, normal, texel colour, ray)
//   1 lane / hit                 the whole-bundle decision (rt::bundle_classify) from the hit's shadow origin; the undecided
//                                are packed again
//   1 lane / undecided hit       truncated mt19937 (mt[397] from the seed table) at depth 1 → the S disk sample positions in LDS
//   1 lane / (undecided hit, light sample)   exact any-hit test on the candidates → lit count by ballot
//                                (decision, packing and pass loop mirror resolve_shadow_bundles at depth 1 in a copy of the pass's own;
//                                the ray loop is count_item_rays)
//   1 lane / hit                 shade level 1; then the rest of its chain sequentially — reflect, closest hit over all meshes,
//                                visibility, shade, to max_bounces (a tenth of the weight per level, a minority of the hits) —
//                                and the fold back to front from a per-lane stack; the colour returns through LDS
//   1 lane / pixel               the planes: 16 bytes per store where rows and alignment allow
// ---------------------------------------------------------------------------------------------
// The meshes a reflection ray of the tile can meet, conservatively: lane m of the calling wave tests mesh m.  With N = (0, 1, 0)
// the reflected direction R is the camera ray's direction D with its y component negated, so the point P + s R is the mirror
// image in the plane of P + s D — the camera ray continued beyond the plane.  A reflection ray therefore meets a box B only
// if the camera ray's LINE meets B mirrored about y = g, and a line through the camera meets a box in front of it only if the
// pixel lies in the box's image: inside the bounding rectangle of its eight projected corners.  The ray really leaves
// P + (0, 1e-3, 0), a parallel line 1e-3 away: the mirrored box (of a posed mesh: of its padded bounding sphere) is inflated by
// 2e-3 + 16 slacks on every side, orders above the float error of R and P; the rectangle takes a relative 1e-3, and the tile
// the two pixels of mesh_touches_tile.  Every other case keeps the mesh: a corner at or behind the camera plane, cull_ok == 0,
// 64 meshes or more, a negative sphere radius, non-finite values (every comparison is written to fail open).
__device__ __forceinline__ unsigned long long reflection_tile_mask(const SceneView& sc, const mcrt_config& cfg, const TileGeom& t, const float aspect,
                                                                   const float g, const bool cull, const int lane) {
    const int n = sc.n_meshes;
    if (n <= 0) return 0ull;
    const unsigned long long all = n < 64 ? (1ull << n) - 1ull : ~0ull;
    if (!cull || sc.hdr->cull_ok == 0 || n >= 64) return all;
    const float slack = sc.hdr->mask_slack;
    const float W = static_cast<float>(cfg.width), H = static_cast<float>(cfg.height);
    // tile extent padded by 2 pixels, in the units of FlatMesh::screen (x: (2u-1)*aspect, y: 1-2v, +y up), as mesh_touches_tile
    const float tu0 = (2.0f * (static_cast<float>(t.x) - 2.0f) / W - 1.0f) * aspect - 1e-3f * aspect - 1e-3f;
    const float tu1 = (2.0f * (static_cast<float>(t.x + t.w) + 2.0f) / W - 1.0f) * aspect + 1e-3f * aspect + 1e-3f;
    const float tv1 = 1.0f - 2.0f * (static_cast<float>(t.y) - 2.0f) / H + 2e-3f;
    const float tv0 = 1.0f - 2.0f * (static_cast<float>(t.y + t.h) + 2.0f) / H - 2e-3f;
    const V3 pos = ld3(sc.hdr->cam_pos), fwd = ld3(sc.hdr->cam_fwd), right = ld3(sc.hdr->cam_right), up = ld3(sc.hdr->cam_up);
    const float inv_h = 1.0f / sc.hdr->cam_half_h;  // cull_ok: finite, in (1e-4, 1e4)
    bool touch = lane < n;
    if (touch) {
        const FlatMesh& m = sc.meshes[lane];
        if (m.flags & MESH_EMPTY) {
            touch = false;  // intersection.cpp:205: never hit
        } else {
            V3 lo = ld3(m.lo), hi = ld3(m.hi);
            bool ok = true;
            if (m.flags & MESH_ROTATED) {
                const float r = m.sphere[3];
                ok = r >= 0.0f;
                lo = mk(m.sphere[0] - r, m.sphere[1] - r, m.sphere[2] - r);
                hi = mk(m.sphere[0] + r, m.sphere[1] + r, m.sphere[2] + r);
            }
            const float pad = 2e-3f + 16.0f * slack;
            // mirrored about y = g and inflated
            const V3 blo = mk(lo.x - pad, g + (g - hi.y) - pad, lo.z - pad), bhi = mk(hi.x + pad, g + (g - lo.y) + pad, hi.z + pad);
            float u0 = kFltMax, u1 = -kFltMax, v0 = kFltMax, v1 = -kFltMax;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const V3 rel = mk(((c & 1) ? bhi.x : blo.x) - pos.x, ((c & 2) ? bhi.y : blo.y) - pos.y, ((c & 4) ? bhi.z : blo.z) - pos.z);
                const float zc = dot(rel, fwd), xc = dot(rel, right), yc = dot(rel, up);
                const float extent = __builtin_fabsf(rel.x) + __builtin_fabsf(rel.y) + __builtin_fabsf(rel.z);
                ok = ok && zc > 1e-3f * (1.0f + extent);  // a corner at or behind the camera plane: no bound
                const float nu = xc / zc * inv_h, nv = yc / zc * inv_h;
                ok = ok && __builtin_fabsf(nu) < 1e30f && __builtin_fabsf(nv) < 1e30f;  // (false for a NaN, which fmin / fmax would drop)
                u0 = __builtin_fminf(u0, nu), u1 = __builtin_fmaxf(u1, nu), v0 = __builtin_fminf(v0, nv), v1 = __builtin_fmaxf(v1, nv);
            }
            if (ok) {
                const float mg = 1e-3f * (1.0f + __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(u0), __builtin_fabsf(u1)), __builtin_fmaxf(__builtin_fabsf(v0), __builtin_fabsf(v1))));
                const bool out = (u1 + mg < tu0) | (u0 - mg > tu1) | (v1 + mg < tv0) | (v0 - mg > tv1);
                touch = !out;
            }
        }
    }
    return __ballot(touch);
}
// visibility term of a hit below level 1, sequential form (rt::hit_visibility with the stream seeded from the device's table)
template <class SV>
__device__ __forceinline__ float chain_visibility(const SceneView& scg, const SV& sc, const uint32_t* __restrict__ seed_table, const Hit& hit, const int depth,
                                                  const int S, const bool soft) {
    const V3 lpos = ld3(scg.hdr->light_pos);
    if (!soft) return in_shadow(sc, hit.p, S > 1 ? hit.n : normalize(hit.n), lpos) ? 0.0f : 1.0f;  // shading.cpp:31 / :76-80
    MtShort rng;
    const uint32_t seed = shadow_seed(hit.p, depth);
    const uint32_t slot = seed + kSeedWindowHalf;
    if (seed_table && slot < kSeedWindow)
        rng.seed_known(seed, seed_table[slot]);
    else
        rng.seed(seed);
    const LightFrame frame = light_frame(scg, hit.p);
    int lit = 0;
    for (int i = 0; i < S; ++i) {
        const float d0 = rng.uniform();
        const float d1 = rng.uniform();
        if (!in_shadow(sc, hit.p, hit.n, light_sample_on_frame(scg, frame, d0, d1))) ++lit;
    }
    return static_cast<float>(lit) / static_cast<float>(S);
}
template <int kView>
__device__ __forceinline__ void reflection_body(const ReflectionFrame& __restrict__ f, const ReflectionShape& __restrict__ sh) {
    extern __shared__ __align__(16) unsigned char s_dyn[];  // [scene tables][ReflectionArea][positions: pass x S x 3 floats]
    __shared__ int s_wcnt[kBlock / 64];
    const SceneView scg = view_of(f.scene);
    const mcrt_config& cfg = sh.tiles.cfg;
    const int tid = threadIdx.x, lane = tid & 63;
    const float aspect = static_cast<float>(cfg.width) / static_cast<float>(cfg.height);
    const float g = f.ground_y;
    const int S = sh.samples;
    const int max_b = sh.max_bounces;
    const bool raw_normal = S > 1;
    const V3 N = mk(0.0f, 1.0f, 0.0f);
    constexpr bool kPosed = kView != kViewLdsUnposed;
    ReflectionArea& area = *reinterpret_cast<ReflectionArea*>(s_dyn + scene_tables_lds_span(f.lds_face_entries, f.lds_alpha_words));
    float4* s_rec = area.rec;  // plane 0: hit point, ray origin x; 1: normal, origin y; 2: texel colour; 3: ray direction, origin z — then the hit's colour
    const V3 lpos = ld3(scg.hdr->light_pos);
    const float lradius = scg.hdr->light_radius;
    const bool soft = S > 1 && !(lradius < 1e-4f);  // shading.cpp:31: otherwise the one isInShadow ray towards the light's centre
    const float R = soft ? lradius : 0.0f;
    const uint32_t pairs = soft ? static_cast<uint32_t>(S) : 1u;  // rays per hit
    const uint32_t pass = static_cast<uint32_t>(sh.pass);
    unsigned long long* s_cand = area.sh.cand;
    unsigned long long* s_ins = area.sh.ins;
    uint32_t* s_lit = area.sh.lit;
    uint32_t* s_und = area.sh.und;
    float* s_pos = reinterpret_cast<float*>(&area + 1);
    const bool quad_rows = (cfg.width & 3) == 0 && (cfg.tile_size & 3) == 0;
    const bool quads_dist = quad_rows && (reinterpret_cast<uintptr_t>(f.distance) & 15u) == 0;
    const bool quads_u8 = quad_rows && (reinterpret_cast<uintptr_t>(f.rgba8) & 15u) == 0;
    const bool vec_rgba = (reinterpret_cast<uintptr_t>(f.rgba) & 15u) == 0;
    const bool word_u8 = (reinterpret_cast<uintptr_t>(f.rgba8) & 3u) == 0;
    const float* bgc = scg.hdr->background;
    const C4 flat_bg{bgc[0], bgc[1], bgc[2], bgc[3]};
    typename ViewSel<kView>::type sc;
    bool staged = false;
    const int n_units = sh.tiles.tiles_x * sh.tiles.tiles_y * sh.tiles.parts;
    for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        UnitPixel up;
        if (!unit_tile(sh.tiles, unit, up)) continue;
        // the same in every wave of the workgroup; max_bounces < 1: the reference returns before it intersects
        const unsigned long long mask = max_b >= 1 ? reflection_tile_mask(scg, cfg, up.tg, aspect, g, sh.cull != 0, lane) : 0ull;
        stage_view_once<kView>(scg, f.lds_face_entries, f.lds_alpha_words, s_dyn, mask != 0ull, sc, staged);
        lane_pixel(cfg, tid, up);
        const bool valid = up.valid;
        const size_t idx = up.idx;
        float dist = kFltMax;
        C4 col{0.0f, 0.0f, 0.0f, 0.0f};
        if (mask != 0ull) {  // uniform
            // ---- a lane per pixel: the ray, the plane point, the reflection ray and its closest hit
            bool is_hit = false;
            Hit h;
            Ray rr{mk(0, 0, 0), mk(0, 0, 0)};
            if (valid) {
                const float u = (static_cast<float>(up.px) + 0.5f) / static_cast<float>(cfg.width);
                const float v = (static_cast<float>(up.py) + 0.5f) / static_cast<float>(cfg.height);
                const Ray ray = camera_ray(scg, u, v, aspect);
                const float t = (g - ray.o.y) / ray.d.y;
                if (ray.d.y != 0.0f && t > 0.0f && t <= kFltMax) {
                    rr = reflect_ray(ray.d, mk(ray.o.x + ray.d.x * t, g, ray.o.z + ray.d.z * t), N);
                    h = hit_scene(sc, rr, mask);
                    is_hit = h.hit;
                }
            }
            int n_hits = 0;
            const int rank = block_rank(is_hit, s_wcnt, n_hits);
            if (is_hit) {
                dist = h.t;
                s_rec[rank] = make_float4(h.p.x, h.p.y, h.p.z, rr.o.x);
                s_rec[kBlock + rank] = make_float4(h.n.x, h.n.y, h.n.z, rr.o.y);
                s_rec[2 * kBlock + rank] = make_float4(h.tex.r, h.tex.g, h.tex.b, h.tex.a);
                s_rec[3 * kBlock + rank] = make_float4(rr.d.x, rr.d.y, rr.d.z, rr.o.z);
            }
            if (n_hits) {  // uniform
                __syncthreads();
                // ---- a lane per hit: the whole-bundle decision of its level-1 shadow rays.  Down to "the counts are complete" this
                // mirrors resolve_shadow_bundles (kernel_common.h) at depth 1 — decision, packing and pass loop are the pass's own
                // copy, the ray loop is the shared count_item_rays: through the whole helper the pose-6 frame at 1080p fell outside
                // the parent's spread in three A/B runs of six (profiles/pass_fold).  A fix to either goes into both
                const bool mine = tid < n_hits;
                Hit hit;
                Ray ray{mk(0, 0, 0), mk(0, 0, 0)};
                hit.hit = true;
                bool undecided = false;
                uint32_t lit = 0u;
                if (mine) {
                    const float4 a = s_rec[tid], b = s_rec[kBlock + tid], c = s_rec[2 * kBlock + tid], d = s_rec[3 * kBlock + tid];
                    hit.p = mk(a.x, a.y, a.z), hit.n = mk(b.x, b.y, b.z), hit.tex = C4{c.x, c.y, c.z, c.w};
                    ray.o = mk(a.w, b.w, d.w), ray.d = mk(d.x, d.y, d.z);
                    const V3 O = hit.p + (raw_normal ? hit.n : normalize(hit.n)) * 1e-3f;
                    unsigned long long cand;
                    const int known = bundle_classify<kPosed>(scg, sc, O, lpos, R, static_cast<int>(pairs), sh.bundle_decisions != 0, cand);
                    undecided = known < 0;
                    s_cand[tid] = cand;
                    s_ins[tid] = (undecided && sh.inside_fast) ? origin_inside_boxes(sc, O, cand) : 0ull;
                    if (!undecided) lit = static_cast<uint32_t>(known);
                }
                s_lit[tid] = 0u;
                int total = 0;
                const int urank = block_rank(undecided, s_wcnt, total);
                if (undecided) s_und[urank] = static_cast<uint32_t>(tid);
                const uint32_t n_und = static_cast<uint32_t>(total);
                if (n_und) __syncthreads();  // uniform
                for (uint32_t u0 = 0; u0 < n_und; u0 += pass) {  // uniform
                    const uint32_t nu = min(pass, n_und - u0);
                    if (u0) __syncthreads();  // the previous pass's rays have read the positions
                    // ---- a lane per undecided hit: its mt19937 stream at depth 1 and the S disk sample positions
                    if (soft && static_cast<uint32_t>(tid) < nu) {
                        const float4 a = s_rec[s_und[u0 + tid]];
                        disk_sample_positions(scg, nullptr, f.seed_table, nullptr, mk(a.x, a.y, a.z), 1, S, s_pos + static_cast<size_t>(tid) * 3 * S);
                    }
                    __syncthreads();
                    // ---- a lane per (undecided hit, light sample): count_item_rays
                    count_item_rays(s_und + u0, nu, pairs, s_lit, [&](const uint32_t k, const uint32_t q) __attribute__((always_inline)) {
                        const float4 a = s_rec[k], b = s_rec[kBlock + k];
                        V3 Nk = mk(b.x, b.y, b.z);
                        if (!raw_normal) Nk = normalize(Nk);
                        const V3 target = soft ? ld3(s_pos + static_cast<size_t>(q) * 3) : lpos;
                        return !in_shadow_masked(sc, mk(a.x, a.y, a.z), Nk, target, s_cand[k], s_ins[k]);
                    });
                }
                if (n_und) __syncthreads();  // the counts are complete
                if (undecided) lit = s_lit[tid];
                // ---- a lane per hit: shade level 1, then the rest of the chain and the fold (rt::trace_from_hit's loop)
                if (mine) {
                    float vis = soft ? static_cast<float>(lit) / static_cast<float>(S) : (lit ? 1.0f : 0.0f);
                    C4 stack[kReflectMaxBounces];
                    int top = 0, depth = 1;
                    C4 tail;
                    for (;;) {
                        const C4 c = shade(scg, hit, normalize(ray.o - hit.p), vis);
                        if (depth >= max_b) {  // no reflection: `shadedColor.a = originalAlpha; return clamp()`
                            tail = clamp4(c);
                            break;
                        }
                        stack[top++] = c;
                        ray = reflect_ray(ray, hit);
                        ++depth;
                        hit = hit_scene<true>(sc, ray, ~0ull);
                        if (!hit.hit) {  // bounced ray missed → flat scene.backgroundColor (:94-102, depth > 0)
                            tail = flat_bg;
                            break;
                        }
                        vis = chain_visibility(scg, sc, f.seed_table, hit, depth, S, soft);
                    }
                    while (top > 0) tail = fold_reflection(stack[--top], tail);
                    s_rec[3 * kBlock + tid] = make_float4(tail.r, tail.g, tail.b, tail.a);  // (record tid is this lane's alone by now)
                }
                __syncthreads();
                if (is_hit) {
                    const float4 c = s_rec[3 * kBlock + rank];
                    col = C4{c.x, c.y, c.z, c.w};
                }
                // (the next unit writes its records behind the two barriers of its block_rank)
            }
        }
        // ---- a lane per pixel: the planes
        if (f.distance) store_plane(f.distance, quads_dist, valid, lane, idx, dist);
        if (f.rgba && valid) {
            if (vec_rgba) {
                reinterpret_cast<float4*>(f.rgba)[idx] = make_float4(col.r, col.g, col.b, col.a);
            } else {
                float* o = f.rgba + idx * 4;
                o[0] = col.r, o[1] = col.g, o[2] = col.b, o[3] = col.a;
            }
        }
        if (f.rgba8) {
            const uchar4 q = quantize_pixel(make_float4(col.r, col.g, col.b, col.a));
            const uint32_t w = static_cast<uint32_t>(q.x) | (static_cast<uint32_t>(q.y) << 8) | (static_cast<uint32_t>(q.z) << 16) | (static_cast<uint32_t>(q.w) << 24);
            if (quads_u8) {  // lanes 4k .. 4k+3 hold four neighbours of one row, all valid or none
                const uint32_t w1 = __shfl_down(w, 1), w2 = __shfl_down(w, 2), w3 = __shfl_down(w, 3);
                if (valid && (lane & 3) == 0) *reinterpret_cast<uint4*>(f.rgba8 + idx * 4) = make_uint4(w, w1, w2, w3);
            } else if (valid) {
                if (word_u8) {
                    *reinterpret_cast<uint32_t*>(f.rgba8 + idx * 4) = w;
                } else {
                    uint8_t* o = f.rgba8 + idx * 4;
                    o[0] = q.x, o[1] = q.y, o[2] = q.z, o[3] = q.w;
                }
            }
        }
    }
}
template <int kView>
__global__ __launch_bounds__(kBlock, kGroundWaves) void reflection_kernel(const ReflectionFrame f, const ReflectionShape sh) {
    reflection_body<kView>(f, sh);
}
using ReflectionTable = const __attribute__((address_space(4))) ReflectionFrame*;
template <int kView>
__global__ __launch_bounds__(kBlock, kGroundWaves) void reflection_batch_kernel(ReflectionTable table, const ReflectionShape sh) {
    reflection_body<kView>(*(const ReflectionFrame*)(table + blockIdx.y), sh);
}

// ---------------------------------------------------------------------------------------------
// light layers (kernels.h: ShadeFrame): what the light does on the figure itself, at the geometry layers' primary hit — the
// visibility term shade() multiplies diffuse and specular by (computeSoftShadow at depth 0, or shade()'s own isInShadow test),
// computeAO, and shade() before ambient occlusion and the bounces are folded in.  Two kernels, so that the AO loop's any-hit
// test and the bundle classification do not share a register budget.  No workspace.
// `shade` (visibility and direct), a workgroup per 256 pixels of a screen tile (grid-stride), in phases handed over through LDS:
//   1 lane / mesh (every wave)   the geometry layers' tile mask: a tile nothing can touch gets the miss constants and forms no ray
//   1 lane / pixel               ray, closest hit among the tile's meshes; the hits are packed onto the block's first lanes as
//                                records in LDS (point, normal, texel colour)
//   1 lane / hit                 the whole-bundle decision (rt::bundle_classify) from the hit's shadow origin; the undecided
//                                are packed again
//   1 lane / undecided hit       truncated mt19937 (mt[397] from the seed table) at depth 0 → the S disk sample positions in LDS
//   1 lane / (undecided hit, light sample)   exact any-hit test on the candidates → lit count by ballot
//                                (the decision and these two phases: resolve_shadow_bundles at depth 0)
//   1 lane / hit                 visibility = lit / S (one ray in the hard modes), shade; both return through LDS
//   1 lane / pixel               the planes: 16 bytes per store where rows and alignment allow
// `occlusion`: the same culling, ray and packing, then the steps of `ao` (render_kernels.hip):
//   1 lane / hit                 the meshes a ray of its hemisphere can meet within the radius (rt::hemisphere_candidates); hits
//                                without one are done at 1.0, the rest are packed again
//   1 lane / packed hit          truncated mt19937 (mt[397] from the device's table of all seeds where a render has built it,
//                                else the recurrence), A cosine-weighted directions, the any-hit test, the count in a register
//                                (record_occlusion over kernel_common.h's AoStream)
// ---------------------------------------------------------------------------------------------
// the pixel-centre ray's closest hit among the meshes of mesh_mask
template <class SV>
__device__ __forceinline__ Hit pixel_hit(const SceneView& scg, const SV& sc, const mcrt_config& cfg, const float aspect, const int px, const int py,
                                         const unsigned long long mesh_mask) {
    const float u = (static_cast<float>(px) + 0.5f) / static_cast<float>(cfg.width);
    const float v = (static_cast<float>(py) + 0.5f) / static_cast<float>(cfg.height);
    return hit_scene(sc, camera_ray(scg, u, v, aspect), mesh_mask);
}
// The first phase of `shade`, `occlusion` and `shade_lights`, a lane per pixel: the pixel-centre ray's closest hit among the
// tile's meshes; the hits are packed onto the block's first lanes as records in LDS — plane 0 the point, plane 1 the normal
// and, where kColour, plane 2 the texel colour.  COLLECTIVE (the two barriers of block_rank: the records are read behind one
// more): all 256 threads reach it under uniform control flow.
struct PixelHits {
    bool is_hit;  // this lane's pixel has a hit,
    int rank;     // whose record this is
    int n_hits;   // the workgroup's records
    float alpha;  // the hit's texel alpha
};
template <bool kColour, class SV>
__device__ __forceinline__ PixelHits pack_pixel_hits(const SceneView& scg, const SV& sc, const mcrt_config& cfg, const float aspect, const UnitPixel& up,
                                                     const unsigned long long mask, float4* s_rec, int* s_wcnt) {
    PixelHits ph{false, 0, 0, 0.0f};
    Hit h;
    if (up.valid) {
        h = pixel_hit(scg, sc, cfg, aspect, up.px, up.py, mask);
        ph.is_hit = h.hit;
    }
    ph.rank = block_rank(ph.is_hit, s_wcnt, ph.n_hits);
    if (ph.is_hit) {
        s_rec[ph.rank] = make_float4(h.p.x, h.p.y, h.p.z, 0.0f);
        s_rec[kBlock + ph.rank] = make_float4(h.n.x, h.n.y, h.n.z, 0.0f);
        if constexpr (kColour) s_rec[2 * kBlock + ph.rank] = make_float4(h.tex.r, h.tex.g, h.tex.b, h.tex.a);
        ph.alpha = h.tex.a;
    }
    return ph;
}
// resolve_shadow_bundles' accessor over records in LDS whose plane 0 holds the point and plane 1 the normal (`shade`, `bake_shade`):
// computeSoftShadow takes the normal as it is (raw), shade()'s own test normalises it (shading.cpp:76-80)
struct RecordPoint {
    const float4* rec;
    bool raw_normal;
    __device__ __forceinline__ void operator()(const uint32_t k, V3& P, V3& N) const {
        const float4 a = rec[k], b = rec[kBlock + k];
        P = mk(a.x, a.y, a.z), N = mk(b.x, b.y, b.z);
        if (!raw_normal) N = normalize(N);
    }
};
template <int kView>
__device__ __forceinline__ void shade_body(const ShadeFrame& __restrict__ f, const ShadeShape& __restrict__ sh) {
    extern __shared__ __align__(16) unsigned char s_dyn[];  // [scene tables][ShadeArea][positions: pass x S x 3 floats]
    __shared__ int s_wcnt[kBlock / 64];
    const SceneView scg = view_of(f.scene);
    const mcrt_config& cfg = sh.tiles.cfg;
    const int tid = threadIdx.x, lane = tid & 63;
    const float aspect = static_cast<float>(cfg.width) / static_cast<float>(cfg.height);
    const V3 cam = ld3(scg.hdr->cam_pos);  // the origin of every pixel-centre ray (rt::camera_ray)
    const int S = sh.samples;
    const bool raw_normal = S > 1;
    constexpr bool kPosed = kView != kViewLdsUnposed;
    ShadeArea& area = *reinterpret_cast<ShadeArea*>(s_dyn + scene_tables_lds_span(f.lds_face_entries, f.lds_alpha_words));
    float4* s_rec = area.rec;      // plane 0: hit point; 1: normal; 2: texel colour — then the hit's colour
    uint32_t* s_lit = area.sh.lit;  // lit counts — then the hit's visibility, bit-cast
    const ShadowBundles sb = shadow_bundles(header_light(scg), S, sh.pass, sh.bundle_decisions, sh.inside_fast, f.seed_table, area.sh.cand, area.sh.ins, area.sh.lit, area.sh.und,
                                            reinterpret_cast<float*>(&area + 1), s_wcnt);
    const bool quads_vis = (cfg.width & 3) == 0 && (cfg.tile_size & 3) == 0 && (reinterpret_cast<uintptr_t>(f.visibility) & 15u) == 0;
    const bool vec_direct = (reinterpret_cast<uintptr_t>(f.direct) & 15u) == 0;
    typename ViewSel<kView>::type sc;
    bool staged = false;
    const int n_units = sh.tiles.tiles_x * sh.tiles.tiles_y * sh.tiles.parts;
    for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        UnitPixel up;
        if (!unit_pixel(sh.tiles, unit, tid, up)) continue;
        const unsigned long long mask = layers_tile_mask(scg, cfg, up.tg, aspect, lane);  // the same in every wave of the workgroup
        stage_view_once<kView>(scg, f.lds_face_entries, f.lds_alpha_words, s_dyn, mask != 0ull, sc, staged);
        float vis = 1.0f;
        C4 col{0.0f, 0.0f, 0.0f, 0.0f};
        if (mask != 0ull) {  // uniform
            // ---- a lane per pixel: the ray and its closest hit, packed
            const PixelHits ph = pack_pixel_hits<true>(scg, sc, cfg, aspect, up, mask, s_rec, s_wcnt);
            if (ph.n_hits) {  // uniform
                __syncthreads();
                // ---- a lane per hit: its record, then resolve_shadow_bundles over its shadow rays (depth 0)
                const bool mine = tid < ph.n_hits;
                Hit hit;
                hit.hit = true;
                uint32_t lit = 0u;
                V3 O = mk(0, 0, 0);
                if (mine) {
                    const float4 a = s_rec[tid], b = s_rec[kBlock + tid], c = s_rec[2 * kBlock + tid];
                    hit.p = mk(a.x, a.y, a.z), hit.n = mk(b.x, b.y, b.z), hit.tex = C4{c.x, c.y, c.z, c.w};
                    O = hit.p + (raw_normal ? hit.n : normalize(hit.n)) * 1e-3f;
                }
                resolve_shadow_bundles<kPosed>(scg, sc, sb, header_light(scg), mine, O, ~0ull, 0, RecordPoint{s_rec, raw_normal}, lit);
                // ---- a lane per hit: the visibility term and shade (raytracer.cpp:107-117)
                if (mine) {
                    const float v = bundle_visibility(sb, lit);
                    const C4 c = shade(scg, hit, normalize(cam - hit.p), v);
                    s_lit[tid] = __float_as_uint(v);  // (entry and record tid are this lane's alone by now)
                    s_rec[2 * kBlock + tid] = make_float4(c.r, c.g, c.b, c.a);
                }
                __syncthreads();
                if (ph.is_hit) {
                    const float4 c = s_rec[2 * kBlock + ph.rank];
                    vis = __uint_as_float(s_lit[ph.rank]);
                    col = C4{c.x, c.y, c.z, c.w};
                }
                // (the next unit writes its records behind the two barriers of its block_rank)
            }
        }
        // ---- a lane per pixel: the planes
        if (f.visibility) store_plane(f.visibility, quads_vis, up.valid, lane, up.idx, vis);
        if (f.direct && up.valid) {
            if (vec_direct) {
                reinterpret_cast<float4*>(f.direct)[up.idx] = make_float4(col.r, col.g, col.b, col.a);
            } else {
                float* o = f.direct + up.idx * 4;
                o[0] = col.r, o[1] = col.g, o[2] = col.b, o[3] = col.a;
            }
        }
    }
}
template <int kView>
__global__ __launch_bounds__(kBlock, kGroundWaves) void shade_kernel(const ShadeFrame f, const ShadeShape sh) {
    shade_body<kView>(f, sh);
}
using ShadeTable = const __attribute__((address_space(4))) ShadeFrame*;
template <int kView>
__global__ __launch_bounds__(kBlock, kGroundWaves) void shade_batch_kernel(ShadeTable table, const ShadeShape sh) {
    shade_body<kView>(*(const ShadeFrame*)(table + blockIdx.y), sh);
}
// computeAO's value at the point of record k by the lane that owns it (`ao`, step 3): its AoStream traced in place against the
// record's candidates, the count in a register
template <class SV>
__device__ __forceinline__ float record_occlusion(const SV& sc, const uint32_t* __restrict__ seed_table_full, const float4* s_rec, const uint32_t k,
                                                  const unsigned long long cand, const bool inside_fast, const float radius, const int A) {
    const float4 a = s_rec[k], b = s_rec[kBlock + k];
    const V3 P = mk(a.x, a.y, a.z), N = normalize(mk(b.x, b.y, b.z));
    const V3 O = P + N * 1e-3f;
    const unsigned long long inside = inside_fast ? origin_inside_boxes(sc, O, cand) : 0ull;  // every ray of the point starts there
    uint32_t occluded = 0;
    AoStream ao(seed_table_full, P, N);
    for (int i = 0; i < A; ++i)
        if (any_hit_masked(sc, Ray{O, ao.next()}, radius, cand, inside)) ++occluded;
    return 1.0f - static_cast<float>(occluded) / static_cast<float>(A);  // raytracer.cpp:77
}
template <int kView>
__device__ __forceinline__ void occlusion_body(const ShadeFrame& __restrict__ f, const ShadeShape& __restrict__ sh) {
    extern __shared__ __align__(16) unsigned char s_dyn[];  // [scene tables][OcclusionArea]
    __shared__ int s_wcnt[kBlock / 64];
    const SceneView scg = view_of(f.scene);
    const mcrt_config& cfg = sh.tiles.cfg;
    const int tid = threadIdx.x, lane = tid & 63;
    const float aspect = static_cast<float>(cfg.width) / static_cast<float>(cfg.height);
    const int A = sh.ao_samples;
    const float radius = sh.ao_radius;
    constexpr bool kPosed = kView != kViewLdsUnposed;
    OcclusionArea& area = *reinterpret_cast<OcclusionArea*>(s_dyn + scene_tables_lds_span(f.lds_face_entries, f.lds_alpha_words));
    float4* s_rec = area.rec;  // plane 0: hit point; 1: normal
    unsigned long long* s_mask = area.mask;
    uint32_t* s_list = area.list;
    float* s_val = area.val;
    const bool quads = (cfg.width & 3) == 0 && (cfg.tile_size & 3) == 0 && (reinterpret_cast<uintptr_t>(f.occlusion) & 15u) == 0;
    typename ViewSel<kView>::type sc;
    bool staged = false;
    const int n_units = sh.tiles.tiles_x * sh.tiles.tiles_y * sh.tiles.parts;
    for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        UnitPixel up;
        if (!unit_pixel(sh.tiles, unit, tid, up)) continue;
        const unsigned long long mask = layers_tile_mask(scg, cfg, up.tg, aspect, lane);  // the same in every wave of the workgroup
        stage_view_once<kView>(scg, f.lds_face_entries, f.lds_alpha_words, s_dyn, mask != 0ull, sc, staged);
        float occ = 1.0f;
        if (mask != 0ull) {  // uniform
            // ---- a lane per pixel: the ray and its closest hit, packed
            const PixelHits ph = pack_pixel_hits<false>(scg, sc, cfg, aspect, up, mask, s_rec, s_wcnt);
            if (ph.n_hits) {  // uniform
                __syncthreads();
                // ---- a lane per hit: the meshes a ray of its hemisphere can meet (`ao`, step 1)
                bool traced = false;
                if (tid < ph.n_hits) {
                    const float4 a = s_rec[tid], b = s_rec[kBlock + tid];
                    const V3 P = mk(a.x, a.y, a.z), N = normalize(mk(b.x, b.y, b.z));
                    const unsigned long long cand = hemisphere_candidates<kPosed>(scg, P + N * 1e-3f, N, radius);
                    s_mask[tid] = cand;
                    traced = cand != 0ull || scg.n_meshes > 64;  // meshes beyond the mask are tested per ray
                    if (!traced) s_val[tid] = 1.0f;  // 0 occluded
                }
                int total = 0;
                const int trank = block_rank(traced, s_wcnt, total);
                if (traced) s_list[trank] = static_cast<uint32_t>(tid);
                __syncthreads();
                // ---- a lane per traced hit: record_occlusion
                if (tid < total) {
                    const uint32_t k = s_list[tid];
                    s_val[k] = record_occlusion(sc, f.seed_table_full, s_rec, k, s_mask[k], sh.inside_fast != 0, radius, A);
                }
                __syncthreads();
                if (ph.is_hit) occ = s_val[ph.rank];
                // (the next unit writes its records behind the two barriers of its block_rank)
            }
        }
        // ---- a lane per pixel: the plane
        store_plane(f.occlusion, quads, up.valid, lane, up.idx, occ);
    }
}
template <int kView>
__global__ __launch_bounds__(kBlock, kGroundWaves) void occlusion_kernel(const ShadeFrame f, const ShadeShape sh) {
    occlusion_body<kView>(f, sh);
}
template <int kView>
__global__ __launch_bounds__(kBlock, kGroundWaves) void occlusion_batch_kernel(ShadeTable table, const ShadeShape sh) {
    occlusion_body<kView>(*(const ShadeFrame*)(table + blockIdx.y), sh);
}

// ---------------------------------------------------------------------------------------------
// light bake (kernels.h: BakeFrame; include/mcrt.h, "light bake"): the light layers' terms per TEXEL of the scene's pool, at
// the q x q sub-sample points of the texel on its owner face — no camera, no tile, no culling.  Two kernels, for the reason of
// the light layers.  No workspace.
// `bake_shade` (visibility and direct), a workgroup per 256 consecutive pool texels (grid-stride), in phases handed over through LDS:
//   1 lane / texel               owner face by a binary search of the handle's face list, texel colour; position and normal
//                                planes; the LIVE texels (an owner, alpha != 0) are packed onto the block's first lanes as
//                                records in LDS (owner face, texel and size; colour)
//   then per sub-sample (j outer, i inner), the steps of `shade` with the sub-sample's P, N in place of the hit:
//   1 lane / live texel          P, N; the whole-bundle decision from P + N * 1e-3f; the undecided are packed again
//   1 lane / undecided point     truncated mt19937 at depth 0 → the S disk sample positions in LDS
//   1 lane / (undecided point, light sample)   exact any-hit test on the candidates → lit count by ballot
//                                (the decision and these two phases: resolve_shadow_bundles at depth 0)
//   1 lane / live texel          visibility = lit / S (one ray in the hard modes), shade with the view vector N; both are
//                                ADDED to the lane's sums in the order the header defines
//   1 lane / texel               the means return through LDS; the planes: 16 bytes per store where the alignment allows
// `bake_occlusion`: the same lookup and packing, then per sub-sample the steps of `occlusion`.
// ---------------------------------------------------------------------------------------------
struct BakeTexel {  // a pool texel on its owner face
    int code;       // mesh * 8 + face slot; -1: no face references the texel
    int tx, ty, w, h;
};
__device__ __forceinline__ BakeTexel bake_owner(const BakeFace* __restrict__ faces, const int n_faces, const int texel) {
    int lo = 0, hi = n_faces;  // the faces before `lo` start at or before the texel, those from `hi` on behind it
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (faces[mid].tex_off <= texel)
            lo = mid + 1;
        else
            hi = mid;
    }
    BakeTexel t{-1, -1, -1, 0, 0};
    if (lo > 0) {
        const BakeFace f = faces[lo - 1];
        const int rel = texel - f.tex_off;
        if (rel < f.w * f.h) {
            t.code = f.code, t.w = f.w, t.h = f.h;
            t.ty = rel / f.w;
            t.tx = rel - t.ty * f.w;
        }
    }
    return t;
}
// sub-sample (i, j) of q x q of the texel: the world point and the normal of a front hit there (include/mcrt.h: the inverse of
// face_uv on the face's plane, then hit_scene's forward rotation for a posed mesh)
template <class SV>
__device__ __forceinline__ void bake_point(const SV& sc, const BakeTexel& t, const int i, const int j, const int q, V3& P, V3& N) {
    const int mesh = t.code >> 3, face = t.code & 7;
    const int axis = face < 2 ? 2 : (face < 4 ? 0 : 1);
    const bool neg = face == 0 || face == 3 || face == 5;
    const MeshData m = mesh_lane(sc, mesh);
    const float u = (static_cast<float>(t.tx) + (static_cast<float>(i) + 0.5f) / static_cast<float>(q)) / static_cast<float>(t.w);
    const float v = (static_cast<float>(t.ty) + (static_cast<float>(j) + 0.5f) / static_cast<float>(q)) / static_cast<float>(t.h);
    const V3 lo = m.lo, hi = m.hi, ext = hi - lo;
    V3 p;
    if (axis == 2) {
        const float lx = neg ? (1.0f - u) : u, ly = 1.0f - v;
        p = mk(lo.x + lx * ext.x, lo.y + ly * ext.y, neg ? lo.z : hi.z);
    } else if (axis == 0) {
        const float lz = neg ? u : (1.0f - u), ly = 1.0f - v;
        p = mk(neg ? lo.x : hi.x, lo.y + ly * ext.y, lo.z + lz * ext.z);
    } else {
        const float lx = u, lz = neg ? (1.0f - v) : v;
        p = mk(lo.x + lx * ext.x, neg ? lo.y : hi.y, lo.z + lz * ext.z);
    }
    P = p;
    N = face_normal(axis, neg);
    if (SV::kPosed && (m.flags & MESH_ROTATED)) {
        P = to_world(m, p);
        N = normalize(spin(N, mk(0.0f, 0.0f, 0.0f), (m.flags & MESH_APPLY_X) != 0, m.fwd_x_cos, m.fwd_x_sin, (m.flags & MESH_APPLY_Z) != 0, m.fwd_z_cos,
                           m.fwd_z_sin));
    }
}
// one value per texel into a plane: 16 bytes per four consecutive texels where `quads` (the plane is 16-byte aligned at the
// frame's first texel) and all four are texels of the frame
__device__ __forceinline__ void bake_store_plane(float* __restrict__ plane, const bool quads, const int texel, const int n_texels, const int lane, const float val) {
    const float v1 = __shfl_down(val, 1), v2 = __shfl_down(val, 2), v3 = __shfl_down(val, 3);
    if (quads && (texel | 3) < n_texels) {
        if ((lane & 3) == 0) *reinterpret_cast<float4*>(plane + texel) = make_float4(val, v1, v2, v3);
    } else if (texel < n_texels) {
        plane[texel] = val;
    }
}
__device__ __forceinline__ void bake_store4(float* __restrict__ plane, const bool vec, const int texel, const float4 val) {
    if (vec) {
        reinterpret_cast<float4*>(plane)[texel] = val;
    } else {
        float* o = plane + static_cast<size_t>(texel) * 4;
        o[0] = val.x, o[1] = val.y, o[2] = val.z, o[3] = val.w;
    }
}
// the first phase of both kernels: this lane's texel, its owner and colour, the position and normal planes
struct BakeLane {
    int texel;
    bool valid, live;
    BakeTexel t;
    float4 tex;
};
template <class SV>
__device__ __forceinline__ BakeLane bake_lane(const BakeFrame& __restrict__ f, const SceneView& scg, const SV& sc, const int unit, const int tid, const bool geometry) {
    BakeLane b;
    b.texel = unit * kBlock + tid;
    b.valid = b.texel < f.n_texels;
    b.t = BakeTexel{-1, -1, -1, 0, 0};
    b.tex = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (b.valid) {
        b.t = bake_owner(f.faces, f.n_faces, b.texel);
        b.tex = scg.texels[b.texel];
    }
    const bool owned = b.t.code >= 0;
    b.live = owned && !(b.tex.w == 0.0f);
    if (geometry && b.valid) {
        float4 pos = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nrm = pos;
        if (owned) {
            V3 P, N;
            bake_point(sc, b.t, 0, 0, 1, P, N);
            pos = make_float4(P.x, P.y, P.z, b.live ? 1.0f : 0.0f);
            nrm = make_float4(N.x, N.y, N.z, 0.0f);
        }
        if (f.position) bake_store4(reinterpret_cast<float*>(f.position), (reinterpret_cast<uintptr_t>(f.position) & 15u) == 0, b.texel, pos);
        if (f.normal) bake_store4(reinterpret_cast<float*>(f.normal), (reinterpret_cast<uintptr_t>(f.normal) & 15u) == 0, b.texel, nrm);
    }
    return b;
}
// The packing phase of the bake kernels, a lane per live texel: the live texels go onto the block's first lanes as records in
// LDS (s_own; with `hit`, their colours into s_tex), then lane tid < n_live reads record tid back — the texel on its owner face
// into t and, with `hit`, the colour and whether the owner mesh is an outer layer into *hit (nullptr: `bake_occlusion`, which
// shades nothing).  Returns this lane's rank: the record of its texel, where that is live.
// COLLECTIVE: the two barriers of block_rank and, where the workgroup has live texels, one more in front of the read.
template <class SV>
__device__ __forceinline__ int pack_live_texels(const SV& sc, const BakeLane& b, int4* s_own, float4* s_tex, int* s_wcnt, int& n_live, BakeTexel& t, Hit* hit) {
    const int tid = threadIdx.x;
    const int rank = block_rank(b.live, s_wcnt, n_live);
    if (b.live) {
        if (hit) s_tex[rank] = b.tex;
        s_own[rank] = make_int4(b.t.code, b.t.ty * b.t.w + b.t.tx, b.t.w, b.t.h);
    }
    t = BakeTexel{-1, -1, -1, 0, 0};
    if (n_live) {  // uniform
        __syncthreads();
        if (tid < n_live) {
            const int4 o = s_own[tid];
            t.code = o.x, t.w = o.z, t.h = o.w;
            t.ty = o.y / o.z;
            t.tx = o.y - t.ty * o.z;
            if (hit) {
                const float4 c = s_tex[tid];
                hit->tex = C4{c.x, c.y, c.z, c.w};
                hit->outer = (mesh_lane(sc, o.x >> 3).flags & MESH_OUTER) != 0;
            }
        }
    }
    return rank;
}
template <int kView>
__device__ __forceinline__ void bake_shade_body(const BakeFrame& __restrict__ f, const BakeShape& __restrict__ sh) {
    extern __shared__ __align__(16) unsigned char s_dyn[];  // [scene tables][BakeShadeArea][positions: pass x S x 3 floats]
    __shared__ int s_wcnt[kBlock / 64];
    const int n_units = (f.n_texels + kBlock - 1) / kBlock;
    if (static_cast<int>(blockIdx.x) >= n_units) return;  // (uniform; before the collective staging: the frames of a batch differ in size)
    const SceneView scg = view_of(f.scene);
    const int tid = threadIdx.x, lane = tid & 63;
    const int S = sh.samples, q = sh.grid;
    const bool raw_normal = S > 1;
    constexpr bool kPosed = kView != kViewLdsUnposed;
    BakeShadeArea& area = *reinterpret_cast<BakeShadeArea*>(s_dyn + scene_tables_lds_span(f.lds_face_entries, f.lds_alpha_words));
    float4* s_rec = area.rec;       // plane 0: point; 1: normal
    float4* s_tex = area.tex;       // the live texel's colour — then its mean colour
    int4* s_own = area.own;         // the live texel on its owner face: {mesh * 8 + face, ty * w + tx, w, h}
    uint32_t* s_lit = area.sh.lit;  // lit counts — then the texel's mean visibility, bit-cast
    const ShadowBundles sb = shadow_bundles(header_light(scg), S, sh.pass, sh.bundle_decisions, sh.inside_fast, f.seed_table, area.sh.cand, area.sh.ins, area.sh.lit, area.sh.und,
                                            reinterpret_cast<float*>(&area + 1), s_wcnt);
    const bool quads_vis = (reinterpret_cast<uintptr_t>(f.visibility) & 15u) == 0;
    const bool vec_direct = (reinterpret_cast<uintptr_t>(f.direct) & 15u) == 0;
    typename ViewSel<kView>::type sc;
    bool staged = false;
    stage_view_once<kView>(scg, f.lds_face_entries, f.lds_alpha_words, s_dyn, true, sc, staged);
    for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        // ---- a lane per texel: owner, colour, the geometry planes; the live texels are packed
        const BakeLane b = bake_lane(f, scg, sc, unit, tid, sh.geometry != 0);
        if (!sh.rays) continue;  // uniform: position / normal alone
        float vis = 1.0f;
        C4 col{0.0f, 0.0f, 0.0f, 0.0f};
        int n_live = 0;
        BakeTexel t;
        Hit hit;
        hit.hit = true;
        const int rank = pack_live_texels(sc, b, s_own, s_tex, s_wcnt, n_live, t, &hit);
        if (n_live) {  // uniform
            const bool mine = tid < n_live;
            float vsum = 0.0f;
            C4 csum{0.0f, 0.0f, 0.0f, 0.0f};
            for (int sub = 0; sub < q * q; ++sub) {  // uniform: j outer, i inner
                const int sj = sub / q, si = sub - sj * q;
                // ---- a lane per live texel: the sub-sample's point, then resolve_shadow_bundles over its shadow rays (depth 0)
                uint32_t lit = 0u;
                V3 O = mk(0, 0, 0);
                if (mine) {
                    bake_point(sc, t, si, sj, q, hit.p, hit.n);
                    s_rec[tid] = make_float4(hit.p.x, hit.p.y, hit.p.z, 0.0f);
                    s_rec[kBlock + tid] = make_float4(hit.n.x, hit.n.y, hit.n.z, 0.0f);
                    O = hit.p + (raw_normal ? hit.n : normalize(hit.n)) * 1e-3f;
                }
                resolve_shadow_bundles<kPosed>(scg, sc, sb, header_light(scg), mine, O, ~0ull, 0, RecordPoint{s_rec, raw_normal}, lit);
                // ---- a lane per live texel: the visibility term and shade, added in the defined order
                if (mine) {
                    const float v = bundle_visibility(sb, lit);
                    const C4 c = shade(scg, hit, hit.n, v);
                    if (sub == 0) {
                        vsum = v, csum = c;
                    } else {
                        vsum = vsum + v;
                        csum = C4{csum.r + c.r, csum.g + c.g, csum.b + c.b, csum.a + c.a};
                    }
                }
            }
            if (mine) {
                if (q > 1) {
                    const float d = static_cast<float>(q * q);
                    vsum = vsum / d;
                    csum = C4{csum.r / d, csum.g / d, csum.b / d, csum.a / d};
                }
                s_lit[tid] = __float_as_uint(vsum);  // (entry and record tid are this lane's alone by now)
                s_tex[tid] = make_float4(csum.r, csum.g, csum.b, csum.a);
            }
            __syncthreads();
            if (b.live) {
                const float4 c = s_tex[rank];
                vis = __uint_as_float(s_lit[rank]);
                col = C4{c.x, c.y, c.z, c.w};
            }
            // (the next unit writes its records behind the two barriers of its block_rank)
        }
        // ---- a lane per texel: the planes
        if (f.visibility) bake_store_plane(f.visibility, quads_vis, b.texel, f.n_texels, lane, vis);
        if (f.direct && b.valid) bake_store4(f.direct, vec_direct, b.texel, make_float4(col.r, col.g, col.b, col.a));
    }
}
template <int kView>
__global__ __launch_bounds__(kBlock, kGroundWaves) void bake_shade_kernel(const BakeFrame f, const BakeShape sh) {
    bake_shade_body<kView>(f, sh);
}
using BakeTable = const __attribute__((address_space(4))) BakeFrame*;
template <int kView>
__global__ __launch_bounds__(kBlock, kGroundWaves) void bake_shade_batch_kernel(BakeTable table, const BakeShape sh) {
    bake_shade_body<kView>(*(const BakeFrame*)(table + blockIdx.y), sh);
}
template <int kView>
__device__ __forceinline__ void bake_occlusion_body(const BakeFrame& __restrict__ f, const BakeShape& __restrict__ sh) {
    extern __shared__ __align__(16) unsigned char s_dyn[];  // [scene tables][BakeOcclusionArea]
    __shared__ int s_wcnt[kBlock / 64];
    const int n_units = (f.n_texels + kBlock - 1) / kBlock;
    if (static_cast<int>(blockIdx.x) >= n_units) return;  // (uniform; before the collective staging)
    const SceneView scg = view_of(f.scene);
    const int tid = threadIdx.x, lane = tid & 63;
    const int A = sh.ao_samples, q = sh.grid;
    const float radius = sh.ao_radius;
    constexpr bool kPosed = kView != kViewLdsUnposed;
    BakeOcclusionArea& area = *reinterpret_cast<BakeOcclusionArea*>(s_dyn + scene_tables_lds_span(f.lds_face_entries, f.lds_alpha_words));
    float4* s_rec = area.rec;  // plane 0: point; 1: normal
    int4* s_own = area.own;    // the live texel on its owner face: {mesh * 8 + face, ty * w + tx, w, h}
    unsigned long long* s_mask = area.mask;
    uint32_t* s_list = area.list;
    float* s_val = area.val;
    const bool quads = (reinterpret_cast<uintptr_t>(f.occlusion) & 15u) == 0;
    typename ViewSel<kView>::type sc;
    bool staged = false;
    stage_view_once<kView>(scg, f.lds_face_entries, f.lds_alpha_words, s_dyn, true, sc, staged);
    for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        // ---- a lane per texel: owner, colour, the geometry planes; the live texels are packed
        const BakeLane b = bake_lane(f, scg, sc, unit, tid, sh.geometry != 0);
        float occ = 1.0f;
        int n_live = 0;
        BakeTexel t;
        const int rank = pack_live_texels(sc, b, s_own, nullptr, s_wcnt, n_live, t, nullptr);
        if (n_live) {  // uniform
            const bool mine = tid < n_live;
            float sum = 0.0f;
            for (int sub = 0; sub < q * q; ++sub) {  // uniform: j outer, i inner
                const int sj = sub / q, si = sub - sj * q;
                // ---- a lane per live texel: the sub-sample's point and the meshes a ray of its hemisphere can meet (`ao`, step 1)
                bool traced = false;
                if (mine) {
                    V3 P, Nr;
                    bake_point(sc, t, si, sj, q, P, Nr);
                    s_rec[tid] = make_float4(P.x, P.y, P.z, 0.0f);
                    s_rec[kBlock + tid] = make_float4(Nr.x, Nr.y, Nr.z, 0.0f);
                    const V3 N = normalize(Nr);
                    const unsigned long long cand = hemisphere_candidates<kPosed>(scg, P + N * 1e-3f, N, radius);
                    s_mask[tid] = cand;
                    traced = cand != 0ull || scg.n_meshes > 64;  // meshes beyond the mask are tested per ray
                    if (!traced) s_val[tid] = 1.0f;  // 0 occluded
                }
                int total = 0;
                const int trank = block_rank(traced, s_wcnt, total);
                if (traced) s_list[trank] = static_cast<uint32_t>(tid);
                __syncthreads();
                // ---- a lane per traced point: record_occlusion
                if (tid < total) {
                    const uint32_t k = s_list[tid];
                    s_val[k] = record_occlusion(sc, f.seed_table_full, s_rec, k, s_mask[k], sh.inside_fast != 0, radius, A);
                }
                __syncthreads();
                if (mine) {
                    const float v = s_val[tid];
                    sum = sub == 0 ? v : sum + v;
                }
                // (the next sub-sample writes this lane's own entries; its lists are read behind the barriers of its block_rank)
            }
            if (mine) s_val[tid] = q > 1 ? sum / static_cast<float>(q * q) : sum;
            __syncthreads();
            if (b.live) occ = s_val[rank];
            // (the next unit writes its records behind the two barriers of its block_rank)
        }
        // ---- a lane per texel: the plane
        bake_store_plane(f.occlusion, quads, b.texel, f.n_texels, lane, occ);
    }
}
template <int kView>
__global__ __launch_bounds__(kBlock, kGroundWaves) void bake_occlusion_kernel(const BakeFrame f, const BakeShape sh) {
    bake_occlusion_body<kView>(f, sh);
}
template <int kView>
__global__ __launch_bounds__(kBlock, kGroundWaves) void bake_occlusion_batch_kernel(BakeTable table, const BakeShape sh) {
    bake_occlusion_body<kView>(*(const BakeFrame*)(table + blockIdx.y), sh);
}

// ---------------------------------------------------------------------------------------------
// light layers and bake under extra lights (kernels.h: ShadeLightsFrame, BakeLightsFrame; include/mcrt.h, "light layers and bake
// under extra lights"): `shade` and `bake_shade` with the shadow resolution and the shading once per light of the frame's LightSet —
// shade_at(frame_light(k), ambient .20 for light 0, the header's, and 0 for the others) — on the hit's ONE shadow seed: every
// light's call seeds its engine from the same (point, depth), so all lights see the same draws.  The packing phases
// (pack_pixel_hits, pack_live_texels), the resolver and shade_at are the single-light bodies'; the bodies are kernels of their own
// because K = 0 through them is slower than `shade` / `bake_shade` (profiles/light_multi).  What differs:
//   the loop over the lights k = 0 .. K is uniform per workgroup (K from the frame record) and runs around the COLLECTIVE
//   resolver (kernel_common.h: resolve_shadow_bundles), whose area it reuses from light to light: behind the resolver nothing
//   of the area is read across lanes, and the LDS a launch takes does not grow with K;
//   `shade_lights`: light k's visibility and colour return through LDS per light (plane 2 of the record, {r, g, b, vis}: the texel
//   colour it held is in the hit lane's registers by then, and the next light's write lies behind its resolver's barriers) and
//   the PIXEL lane adds the colours left to right — the additions the definition names — and clamps the sum;
//   `bake_shade_lights`: the texel's lane keeps a sum per light and the sum of the sub-samples' clamped totals in registers
//   (the per-light slots are addressed by unrolled selects, never by index) and hands the means back light by light;
//   a plane of a light the frame lacks (k > K) takes the miss constants.
// ---------------------------------------------------------------------------------------------
// light k of a frame, k uniform: the header's, or entry k - 1 of the record's set (a scalar load, not a select)
__device__ __forceinline__ LightAt frame_light(const SceneView& scg, const LightSet& ls, const int k) {
    if (k == 0) return light_value(header_light(scg));
    const mcrt_light_source& e = ls.extra[k - 1];
    return LightAt{mk(e.position[0], e.position[1], e.position[2]), e.radius, {e.color[0], e.color[1], e.color[2]}};
}
__device__ __forceinline__ void store_rgba(float* __restrict__ plane, const size_t idx, const float4 val) {
    if ((reinterpret_cast<uintptr_t>(plane) & 15u) == 0) {
        reinterpret_cast<float4*>(plane)[idx] = val;
    } else {
        float* o = plane + idx * 4;
        o[0] = val.x, o[1] = val.y, o[2] = val.z, o[3] = val.w;
    }
}
template <int kView>
__device__ __forceinline__ void shade_lights_body(const ShadeLightsFrame& __restrict__ f, const ShadeShape& __restrict__ sh) {
    extern __shared__ __align__(16) unsigned char s_dyn[];  // [scene tables][ShadeArea][positions: pass x S x 3 floats]
    __shared__ int s_wcnt[kBlock / 64];
    const SceneView scg = view_of(f.scene);
    const mcrt_config& cfg = sh.tiles.cfg;
    const int tid = threadIdx.x, lane = tid & 63;
    const float aspect = static_cast<float>(cfg.width) / static_cast<float>(cfg.height);
    const V3 cam = ld3(scg.hdr->cam_pos);
    const int S = sh.samples;
    const int K = min(max(f.lights.n_extra, 0), MCRT_MAX_EXTRA_LIGHTS);  // uniform
    const bool raw_normal = S > 1;
    constexpr bool kPosed = kView != kViewLdsUnposed;
    ShadeArea& area = *reinterpret_cast<ShadeArea*>(s_dyn + scene_tables_lds_span(f.lds_face_entries, f.lds_alpha_words));
    float4* s_rec = area.rec;  // plane 0: hit point; 1: normal; 2: texel colour — then, per light, the hit's {r, g, b, visibility}
    const bool quads_ok = (cfg.width & 3) == 0 && (cfg.tile_size & 3) == 0;
    typename ViewSel<kView>::type sc;
    bool staged = false;
    const int n_units = sh.tiles.tiles_x * sh.tiles.tiles_y * sh.tiles.parts;
    for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        UnitPixel up;
        if (!unit_pixel(sh.tiles, unit, tid, up)) continue;
        const unsigned long long mask = layers_tile_mask(scg, cfg, up.tg, aspect, lane);  // the same in every wave of the workgroup
        stage_view_once<kView>(scg, f.lds_face_entries, f.lds_alpha_words, s_dyn, mask != 0ull, sc, staged);
        // ---- a lane per pixel: the ray and its closest hit; a lane per hit: its record
        bool is_hit = false, mine = false, shaded = false;  // shaded: uniform — the unit holds hits, the lights' loop resolves and shades
        int rank = 0;
        float alpha = 0.0f;  // shade()'s alpha of the pixel's hit: the texel's, clamped
        Hit hit;
        hit.hit = true;
        V3 O = mk(0, 0, 0), view = mk(0, 0, 0);
        if (mask != 0ull) {  // uniform
            const PixelHits ph = pack_pixel_hits<true>(scg, sc, cfg, aspect, up, mask, s_rec, s_wcnt);
            is_hit = ph.is_hit, rank = ph.rank;
            if (is_hit) alpha = sclamp(ph.alpha, 0.0f, 1.0f);
            if (ph.n_hits) {  // uniform
                __syncthreads();
                shaded = true;
                mine = tid < ph.n_hits;
                if (mine) {
                    const float4 a = s_rec[tid], b = s_rec[kBlock + tid], c = s_rec[2 * kBlock + tid];
                    hit.p = mk(a.x, a.y, a.z), hit.n = mk(b.x, b.y, b.z), hit.tex = C4{c.x, c.y, c.z, c.w};
                    O = hit.p + (raw_normal ? hit.n : normalize(hit.n)) * 1e-3f;
                    view = normalize(cam - hit.p);
                }
            }
        }
        // ---- per light slot k: its planes.  A light the frame has (k <= K), in a unit with hits: the resolver and shade; otherwise the
        // miss constants — ONE store site per plane, its values formed right in front of it
        C4 comb{0.0f, 0.0f, 0.0f, 0.0f};
        for (int k = 0; k < kMaxLights; ++k) {  // uniform
            float vis = 1.0f;
            C4 col{0.0f, 0.0f, 0.0f, 0.0f};
            if (shaded && k <= K) {  // uniform: the resolver inside is collective
                const LightAt l = frame_light(scg, f.lights, k);
                const ShadowBundles sb = shadow_bundles(l, S, sh.pass, sh.bundle_decisions, sh.inside_fast, f.seed_table, area.sh.cand, area.sh.ins,
                                                           area.sh.lit, area.sh.und, reinterpret_cast<float*>(&area + 1), s_wcnt);
                // ---- resolve_shadow_bundles over the hits' shadow rays towards light k (depth 0)
                uint32_t lit = 0u;
                resolve_shadow_bundles<kPosed>(scg, sc, sb, l, mine, O, ~0ull, 0, RecordPoint{s_rec, raw_normal}, lit);
                // ---- a lane per hit: light k's visibility term and shade
                if (mine) {
                    const float v = bundle_visibility(sb, lit);
                    const C4 c = shade_at(l, hit, view, k == 0 ? 0.20f : 0.0f, v);
                    s_rec[2 * kBlock + tid] = make_float4(c.r, c.g, c.b, v);  // (record tid is this lane's alone; its colour is in `hit`)
                }
                __syncthreads();
                // ---- a lane per pixel: light k's values, and its term of the sum
                if (is_hit) {
                    const float4 r = s_rec[2 * kBlock + rank];
                    vis = r.w;
                    col = C4{r.x, r.y, r.z, alpha};
                    comb = k == 0 ? col : C4{comb.r + col.r, comb.g + col.g, comb.b + col.b, comb.a};
                }
                // (the next light's record write lies behind the barriers of its resolver's block_rank, the next unit's behind its own)
            }
            float* const pv = f.vis[k];
            float* const pd = f.dir[k];
            if (pv) store_plane(pv, quads_ok && (reinterpret_cast<uintptr_t>(pv) & 15u) == 0, up.valid, lane, up.idx, vis);
            if (pd && up.valid) store_rgba(pd, up.idx, make_float4(col.r, col.g, col.b, col.a));
        }
        if (f.combined && up.valid) {
            comb = clamp4(comb);
            store_rgba(f.combined, up.idx, make_float4(comb.r, comb.g, comb.b, comb.a));
        }
    }
}
template <int kView>
__global__ __launch_bounds__(kBlock, kGroundWaves) void shade_lights_kernel(const ShadeLightsFrame f, const ShadeShape sh) {
    shade_lights_body<kView>(f, sh);
}
using ShadeLightsTable = const __attribute__((address_space(4))) ShadeLightsFrame*;
template <int kView>
__global__ __launch_bounds__(kBlock, kGroundWaves) void shade_lights_batch_kernel(ShadeLightsTable table, const ShadeShape sh) {
    shade_lights_body<kView>(*(const ShadeLightsFrame*)(table + blockIdx.y), sh);
}
template <int kView>
__device__ __forceinline__ void bake_shade_lights_body(const BakeLightsFrame& __restrict__ f, const BakeShape& __restrict__ sh) {
    extern __shared__ __align__(16) unsigned char s_dyn[];  // [scene tables][BakeShadeArea][positions: pass x S x 3 floats]
    __shared__ int s_wcnt[kBlock / 64];
    const int n_units = (f.n_texels + kBlock - 1) / kBlock;
    if (static_cast<int>(blockIdx.x) >= n_units) return;  // (uniform; before the collective staging: the frames of a batch differ in size)
    const SceneView scg = view_of(f.scene);
    const int tid = threadIdx.x, lane = tid & 63;
    const int S = sh.samples, q = sh.grid;
    const int K = min(max(f.lights.n_extra, 0), MCRT_MAX_EXTRA_LIGHTS);  // uniform
    const bool raw_normal = S > 1;
    constexpr bool kPosed = kView != kViewLdsUnposed;
    BakeShadeArea& area = *reinterpret_cast<BakeShadeArea*>(s_dyn + scene_tables_lds_span(f.lds_face_entries, f.lds_alpha_words));
    float4* s_rec = area.rec;       // plane 0: point; 1: normal
    float4* s_tex = area.tex;       // the live texel's colour — then, plane by plane, its means
    int4* s_own = area.own;         // the live texel on its owner face: {mesh * 8 + face, ty * w + tx, w, h}
    uint32_t* s_lit = area.sh.lit;  // lit counts — then the texel's mean alpha, bit-cast
    typename ViewSel<kView>::type sc;
    bool staged = false;
    stage_view_once<kView>(scg, f.lds_face_entries, f.lds_alpha_words, s_dyn, true, sc, staged);
    for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        // ---- a lane per texel: owner, colour, the geometry planes; the live texels are packed
        const BakeLane b = bake_lane(f, scg, sc, unit, tid, sh.geometry != 0);
        if (!sh.rays) continue;  // uniform: position / normal alone
        int n_live = 0;
        BakeTexel t;
        Hit hit;
        hit.hit = true;
        const int rank = pack_live_texels(sc, b, s_own, s_tex, s_wcnt, n_live, t, &hit);
        const bool mine = tid < n_live;
        float vsum[kMaxLights];  // (addressed by unrolled selects alone: registers)
        C4 csum[kMaxLights];
        C4 msum{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < kMaxLights; ++j) vsum[j] = 0.0f, csum[j] = C4{0.0f, 0.0f, 0.0f, 0.0f};
        if (n_live) {  // uniform
            for (int sub = 0; sub < q * q; ++sub) {  // uniform: j outer, i inner
                const int sj = sub / q, si = sub - sj * q;
                // ---- a lane per live texel: the sub-sample's point
                V3 O = mk(0, 0, 0);
                if (mine) {
                    bake_point(sc, t, si, sj, q, hit.p, hit.n);
                    s_rec[tid] = make_float4(hit.p.x, hit.p.y, hit.p.z, 0.0f);
                    s_rec[kBlock + tid] = make_float4(hit.n.x, hit.n.y, hit.n.z, 0.0f);
                    O = hit.p + (raw_normal ? hit.n : normalize(hit.n)) * 1e-3f;
                }
                // (the record of lane tid is read across lanes only behind the barriers of the resolver's block_rank, and the
                // previous sub-sample's last resolver has left nothing to be read)
                C4 comb{0.0f, 0.0f, 0.0f, 0.0f};
                for (int k = 0; k <= K; ++k) {  // uniform: the resolver inside is collective
                    const LightAt l = frame_light(scg, f.lights, k);
                    const ShadowBundles sb = shadow_bundles(l, S, sh.pass, sh.bundle_decisions, sh.inside_fast, f.seed_table, area.sh.cand, area.sh.ins,
                                                               area.sh.lit, area.sh.und, reinterpret_cast<float*>(&area + 1), s_wcnt);
                    uint32_t lit = 0u;
                    resolve_shadow_bundles<kPosed>(scg, sc, sb, l, mine, O, ~0ull, 0, RecordPoint{s_rec, raw_normal}, lit);
                    // ---- a lane per live texel: light k's visibility term and shade, added in the defined order
                    if (mine) {
                        const float v = bundle_visibility(sb, lit);
                        const C4 c = shade_at(l, hit, hit.n, k == 0 ? 0.20f : 0.0f, v);
                        comb = k == 0 ? c : C4{comb.r + c.r, comb.g + c.g, comb.b + c.b, comb.a};
#pragma unroll
                        for (int j = 0; j < kMaxLights; ++j)
                            if (j == k) {
                                if (sub == 0) {
                                    vsum[j] = v, csum[j] = c;
                                } else {
                                    vsum[j] = vsum[j] + v;
                                    csum[j] = C4{csum[j].r + c.r, csum[j].g + c.g, csum[j].b + c.b, csum[j].a + c.a};
                                }
                            }
                    }
                }
                if (mine) {
                    comb = clamp4(comb);
                    msum = sub == 0 ? comb : C4{msum.r + comb.r, msum.g + comb.g, msum.b + comb.b, msum.a + comb.a};
                }
            }
            if (mine) {
                if (q > 1) {
                    const float d = static_cast<float>(q * q);
#pragma unroll
                    for (int j = 0; j < kMaxLights; ++j) {
                        vsum[j] = vsum[j] / d;
                        csum[j] = C4{csum[j].r / d, csum[j].g / d, csum[j].b / d, csum[j].a / d};
                    }
                    msum = C4{msum.r / d, msum.g / d, msum.b / d, msum.a / d};
                }
                s_lit[tid] = __float_as_uint(csum[0].a);  // (entry tid is this lane's alone by now; every light's mean alpha is light 0's)
            }
        }
        // ---- the means return through LDS plane by plane — lights 0 .. K, then the sum — and a lane per texel stores them; a light
        // the frame lacks and a dead texel take the constants
        for (int k = 0; k <= kMaxLights; ++k) {  // uniform
            const bool sum = k == kMaxLights;
            float4 r = make_float4(0.0f, 0.0f, 0.0f, sum ? 0.0f : 1.0f);
            float alpha = 0.0f;
            if (n_live && (sum || k <= K)) {  // uniform
                __syncthreads();  // the previous plane's values have been read (the first: the texel colours)
                if (mine) {
                    float pv = vsum[0];
                    C4 pc = csum[0];
#pragma unroll
                    for (int j = 1; j < kMaxLights; ++j)
                        if (j == k) pv = vsum[j], pc = csum[j];
                    if (sum) pv = msum.a, pc = msum;
                    s_tex[tid] = make_float4(pc.r, pc.g, pc.b, pv);
                }
                __syncthreads();
                if (b.live) {
                    r = s_tex[rank];
                    alpha = __uint_as_float(s_lit[rank]);
                }
            }
            if (sum) {
                if (f.combined && b.valid) bake_store4(f.combined, (reinterpret_cast<uintptr_t>(f.combined) & 15u) == 0, b.texel, r);
            } else {
                float* const pv = f.vis[k];
                float* const pd = f.dir[k];
                if (pv) bake_store_plane(pv, (reinterpret_cast<uintptr_t>(pv) & 15u) == 0, b.texel, f.n_texels, lane, r.w);
                if (pd && b.valid) bake_store4(pd, (reinterpret_cast<uintptr_t>(pd) & 15u) == 0, b.texel, make_float4(r.x, r.y, r.z, alpha));
            }
        }
        // (the next unit writes its records behind the two barriers of its block_rank)
    }
}
template <int kView>
__global__ __launch_bounds__(kBlock, kGroundWaves) void bake_shade_lights_kernel(const BakeLightsFrame f, const BakeShape sh) {
    bake_shade_lights_body<kView>(f, sh);
}
using BakeLightsTable = const __attribute__((address_space(4))) BakeLightsFrame*;
template <int kView>
__global__ __launch_bounds__(kBlock, kGroundWaves) void bake_shade_lights_batch_kernel(BakeLightsTable table, const BakeShape sh) {
    bake_shade_lights_body<kView>(*(const BakeLightsFrame*)(table + blockIdx.y), sh);
}

// ---------------------------------------------------------------------------------------------
// studio shot (kernels.h: ShotFrame): the blend of include/mcrt.h, "studio shot" — the straight-alpha figure over a page that
// carries the ground shadow and the floor reflection — as one streaming pass.  No scene geometry, no LDS, no atomics:
//   1 lane / pixel (grid-stride over the frame's pixels, blockIdx.y = frame)
//     figure and reflection rgba   one 16-byte load each where the plane is 16-byte aligned, else four 4-byte loads
//     visibility, distance and floor occlusion   one 4-byte load each: 256 contiguous bytes per wave (the planes have pixel
//                                  granularity); the occlusion only where the frame has that plane
//     page                         the constant, or rt::background at the pixel centre — u, v by IEEE division
//     out                          one 16-byte store (four 4-byte ones for a plane off a 16-byte boundary) and / or 4 bytes
//                                  of RGBA8 (byte stores for a plane off a 4-byte boundary)
// At most 44 B read and 20 B written per pixel.  The arithmetic is the header's, in its order, one rounding per operation; an
// absent input enters with its miss constant (visibility 1, reflection (0,0,0,0)) through the same operations, which is why a
// shot that skips a pass equals one that ran it.  One body for every entry family (include/mcrt.h, "cut-out"); beyond the
// opaque blend of the plain and _occ entries, which reach it with C = 0 and no bounds, it has
//   C          the shadow's colour with the weight dk = (1 - lit) * (1 - ar).  Where all of C is 0 — uniform per launch —
//              the term is not formed
//   kCutout    the transparent page: the floor is a layer of alpha af = 1 - keep under the figure; af == 0 hands F through
//              untouched, otherwise one division per channel un-premultiplies the sum.  The page is not evaluated
//   bounds     (kCutout only, NULL: none of it runs) per lane the running box of its pixels with out.a > 0 over its trips,
//              one xor-shuffle reduction per wave, the four waves' boxes through 64 bytes of LDS, and from the first lane of
//              a workgroup that saw such a pixel at most four atomics on the frame's entry — one per side its box moves —,
//              which holds {width, height, 0, 0} from a launch ahead in the stream.  Atomics on one cache line queue up, so
//              the workgroups take the frame's chunks from the outside in — 0, last, 1, last but one, ... —: the first ones
//              that see content set the top and the bottom, and the later ones find their box inside the entry
// ---------------------------------------------------------------------------------------------
struct ShotPage {  // what rt::background reads of a scene view
    const FlatHeader* hdr;
};
__device__ __forceinline__ float4 load_rgba(const float* __restrict__ plane, const size_t i, const bool aligned) {
    if (aligned) return reinterpret_cast<const float4*>(plane)[i];
    const float* p = plane + 4 * i;
    return make_float4(p[0], p[1], p[2], p[3]);
}
using ShotTable = const __attribute__((address_space(4))) ShotFrame*;
template <bool kCutout>
__device__ __forceinline__ void shot_body(const ShotFrame& __restrict__ f, const ShotShape& __restrict__ sh, int32_t* __restrict__ bounds) {
    const mcrt_config& cfg = sh.cfg;
    const unsigned width = static_cast<unsigned>(cfg.width);
    const unsigned n_pixels = width * static_cast<unsigned>(cfg.height);  // (the host refuses frames of 2^31 pixels and more)
    const bool fig16 = (reinterpret_cast<uintptr_t>(f.figure) & 15u) == 0;
    const bool ref16 = (reinterpret_cast<uintptr_t>(f.reflection) & 15u) == 0;
    const bool out16 = (reinterpret_cast<uintptr_t>(f.out) & 15u) == 0;
    const bool out8_4 = (reinterpret_cast<uintptr_t>(f.out8) & 3u) == 0;
    const bool page_reference = !kCutout && sh.page == MCRT_PAGE_REFERENCE;
    const ShotPage scene{reinterpret_cast<const FlatHeader*>(f.scene)};
    const UDiv by_width(width);
    const float s = sh.shadow_strength, k = sh.reflectivity, fade = sh.reflection_fade;
    const float cr = sh.shadow_color[0], cg = sh.shadow_color[1], cb = sh.shadow_color[2];
    const bool colored = !(cr == 0.0f && cg == 0.0f && cb == 0.0f);
    int x0 = cfg.width, y0 = cfg.height, x1 = 0, y1 = 0;  // this lane's box: the identities
    unsigned chunk = blockIdx.x;
    if (kCutout && bounds) chunk = (blockIdx.x & 1u) ? gridDim.x - 1u - (blockIdx.x >> 1) : blockIdx.x >> 1;  // from the outside in
    for (unsigned i = chunk * kBlock + threadIdx.x; i < n_pixels; i += gridDim.x * kBlock) {
        const float4 F = load_rgba(f.figure, i, fig16);
        const float vis = f.visibility ? f.visibility[i] : 1.0f;
        const float4 R = f.reflection ? load_rgba(f.reflection, i, ref16) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float shade = s * (1.0f - vis);
        float fd = 1.0f;
        if (fade > 0.0f) {
            const float dR = (f.reflection && f.distance) ? f.distance[i] : kFltMax;
            fd = sclamp(1.0f - dR / fade, 0.0f, 1.0f);
        }
        const float ar = (k * R.w) * fd;
        float lit = 1.0f - shade;
        if (f.occlusion) lit = lit * (1.0f - sh.floor_occlusion * (1.0f - f.occlusion[i]));  // absent: oc = +0, and x * 1.0f is x
        const float keep = lit * (1.0f - ar);
        const float under = 1.0f - F.w;
        float4 o;
        if constexpr (kCutout) {
            const float af = 1.0f - keep;
            o = F;
            if (af != 0.0f) {
                float fr = R.x * ar, fg = R.y * ar, fb = R.z * ar;
                if (colored) {
                    const float dk = (1.0f - lit) * (1.0f - ar);
                    fr = cr * dk + fr, fg = cg * dk + fg, fb = cb * dk + fb;
                }
                const float A = F.w + af * under;
                o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (A > 0.0f) {
                    o.x = (F.x * F.w + fr * under) / A;
                    o.y = (F.y * F.w + fg * under) / A;
                    o.z = (F.z * F.w + fb * under) / A;
                    o.w = A;
                }
            }
            if (bounds && o.w > 0.0f) {
                const unsigned py = by_width.div(i), px = i - py * width;
                x0 = min(x0, static_cast<int>(px)), y0 = min(y0, static_cast<int>(py));
                x1 = max(x1, static_cast<int>(px) + 1), y1 = max(y1, static_cast<int>(py) + 1);
            }
        } else {
            float pr = sh.page_color[0], pg = sh.page_color[1], pb = sh.page_color[2];
            if (page_reference) {
                const unsigned py = by_width.div(i), px = i - py * width;
                const float u = (static_cast<float>(px) + 0.5f) / static_cast<float>(cfg.width);
                const float v = (static_cast<float>(py) + 0.5f) / static_cast<float>(cfg.height);
                const C4 c = background(scene, cfg, u, v);
                pr = c.r, pg = c.g, pb = c.b;
            }
            float fr = pr * keep, fg = pg * keep, fb = pb * keep;
            if (colored) {
                const float dk = (1.0f - lit) * (1.0f - ar);
                fr = fr + cr * dk, fg = fg + cg * dk, fb = fb + cb * dk;
            }
            o.x = F.x * F.w + (fr + R.x * ar) * under;
            o.y = F.y * F.w + (fg + R.y * ar) * under;
            o.z = F.z * F.w + (fb + R.z * ar) * under;
            o.w = 1.0f;
        }
        if (f.out) {
            if (out16) {
                reinterpret_cast<float4*>(f.out)[i] = o;
            } else {
                float* p = f.out + 4 * static_cast<size_t>(i);
                p[0] = o.x, p[1] = o.y, p[2] = o.z, p[3] = o.w;
            }
        }
        if (f.out8) {
            const uchar4 q = quantize_pixel(o);
            if (out8_4) {
                reinterpret_cast<uchar4*>(f.out8)[i] = q;
            } else {
                uint8_t* p = f.out8 + 4 * static_cast<size_t>(i);
                p[0] = q.x, p[1] = q.y, p[2] = q.z, p[3] = q.w;
            }
        }
    }
    if constexpr (kCutout) {
        if (bounds) {  // uniform per launch; every lane of the wave is back here behind its trips
            for (int m = 32; m > 0; m >>= 1) {
                x0 = min(x0, __shfl_xor(x0, m)), y0 = min(y0, __shfl_xor(y0, m));
                x1 = max(x1, __shfl_xor(x1, m)), y1 = max(y1, __shfl_xor(y1, m));
            }
            __shared__ int s_box[kBlock / 64][4];
            if ((threadIdx.x & 63u) == 0) {
                int* mine = s_box[threadIdx.x >> 6];
                mine[0] = x0, mine[1] = y0, mine[2] = x1, mine[3] = y1;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                for (int w = 1; w < kBlock / 64; ++w) {
                    x0 = min(x0, s_box[w][0]), y0 = min(y0, s_box[w][1]);
                    x1 = max(x1, s_box[w][2]), y1 = max(y1, s_box[w][3]);
                }
            }
            if (threadIdx.x == 0 && x1 > 0) {
                // The entry only ever moves outwards, so a value read now, however stale, can make an atomic superfluous but
                // never missing: a workgroup whose box lies inside what it reads adds nothing.  (Unconditional and per wave,
                // the atomics of a 1920 x 1080 frame queue up on the entry's one cache line: 0.2 ms against 0.02 for the blend.)
                const int bx0 = __hip_atomic_load(bounds + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int by0 = __hip_atomic_load(bounds + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int bx1 = __hip_atomic_load(bounds + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int by1 = __hip_atomic_load(bounds + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (x0 < bx0) atomicMin(bounds + 0, x0);
                if (y0 < by0) atomicMin(bounds + 1, y0);
                if (x1 > bx1) atomicMax(bounds + 2, x1);
                if (y1 > by1) atomicMax(bounds + 3, y1);
            }
        }
    }
}
template <bool kCutout>
__global__ __launch_bounds__(kBlock) void shot_kernel(const ShotFrame f, const ShotShape sh, int32_t* bounds) {
    shot_body<kCutout>(f, sh, bounds);
}
template <bool kCutout>
__global__ __launch_bounds__(kBlock) void shot_batch_kernel(ShotTable table, const ShotShape sh, int32_t* bounds) {
    shot_body<kCutout>(*(const ShotFrame*)(table + blockIdx.y), sh, bounds ? bounds + 4 * blockIdx.y : nullptr);
}
__global__ __launch_bounds__(kBlock) void shot_bounds_init_kernel(int32_t* bounds, int n, int width, int height) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;  // a lane per word: the entries need 4-byte alignment only
    if (i < 4u * static_cast<unsigned>(n)) bounds[i] = (i & 3u) == 0 ? width : (i & 3u) == 1 ? height : 0;
}

// ---- host-side launchers (the shapes and LDS sizes they take: render_plan.cpp) ----------------------
// One launch of a tile pass (layers, ground) over the tile grid `tiles`.  arg: the frame, or the device table of n_frames
// frames (blockIdx.y = frame); kernel_of(view tag): the kernel of that variant; dyn: its dynamic LDS, hbm_dyn: the HBM
// variant's (which stages no tables)
template <class Arg, class Shape, class KernelOf>
static hipError_t launch_tile_pass(const Arg& arg, int n_frames, const Shape& shape, const LayersShape& tiles, int view, size_t dyn, size_t hbm_dyn,
                                   hipStream_t stream, KernelOf kernel_of) {
    const long long n_units = static_cast<long long>(tiles.tiles_x) * tiles.tiles_y * tiles.parts;
    if (n_units <= 0 || n_frames <= 0) return hipSuccess;
    if (n_frames > kLayersBatchMaxFrames) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>(n_units < kLayersGrid ? n_units : kLayersGrid), static_cast<unsigned>(n_frames));
    with_view(view, [&](auto v) { hipLaunchKernelGGL(kernel_of(v), grid, dim3(kBlock), decltype(v)::value == kViewHbm ? hbm_dyn : dyn, stream, arg, shape); });
    return hipGetLastError();
}
hipError_t launch_layers(const LayersFrame& f, const LayersShape& shape, int view, hipStream_t stream) {
    return launch_tile_pass(f, 1, shape, shape, view, layers_lds_bytes(f), 0, stream, [](auto v) { return layers_kernel<decltype(v)::value>; });
}
hipError_t launch_layers_batch(const LayersFrame* d_table, int n_frames, const LayersShape& shape, int view, size_t max_dyn, hipStream_t stream) {
    return launch_tile_pass(LayersTable(d_table), n_frames, shape, shape, view, max_dyn, 0, stream, [](auto v) { return layers_batch_kernel<decltype(v)::value>; });
}
// ---- ground shadow (kernels.h): the HBM variant keeps the block's area in dynamic LDS -----------------------
hipError_t launch_ground(const GroundFrame& f, const GroundShape& shape, int view, hipStream_t stream) {
    const size_t dyn = ground_lds_bytes(f, shape);
    return launch_tile_pass(f, 1, shape, shape.tiles, view, dyn, dyn, stream, [](auto v) { return ground_kernel<decltype(v)::value>; });
}
hipError_t launch_ground_batch(const GroundFrame* d_table, int n_frames, const GroundShape& shape, int view, size_t max_dyn, hipStream_t stream) {
    return launch_tile_pass(GroundTable(d_table), n_frames, shape, shape.tiles, view, max_dyn, max_dyn, stream, [](auto v) { return ground_batch_kernel<decltype(v)::value>; });
}
// ---- ground occlusion (kernels.h): as the ground pass, the HBM variant keeps the block's area in dynamic LDS ---------------
static bool ground_occlusion_shape_ok(const GroundOcclusionShape& sh) {  // what the draws and the LDS area are laid out for
    return sh.ao_samples >= 1 && sh.ao_samples <= kLightMaxSamples && sh.pass >= 1 && sh.pass <= kBlock &&
           static_cast<size_t>(sh.pass) * sh.ao_samples * 12 <= static_cast<size_t>(kGroundOccDirBytes);
}
hipError_t launch_ground_occlusion(const GroundOcclusionFrame& f, const GroundOcclusionShape& shape, int view, hipStream_t stream) {
    if (!ground_occlusion_shape_ok(shape)) return hipErrorInvalidValue;
    const size_t dyn = ground_occlusion_lds_bytes(f, shape);
    return launch_tile_pass(f, 1, shape, shape.tiles, view, dyn, dyn, stream, [](auto v) { return ground_occlusion_kernel<decltype(v)::value>; });
}
hipError_t launch_ground_occlusion_batch(const GroundOcclusionFrame* d_table, int n_frames, const GroundOcclusionShape& shape, int view, size_t max_dyn,
                                         hipStream_t stream) {
    if (!ground_occlusion_shape_ok(shape)) return hipErrorInvalidValue;
    return launch_tile_pass(GroundOcclusionTable(d_table), n_frames, shape, shape.tiles, view, max_dyn, max_dyn, stream,
                            [](auto v) { return ground_occlusion_batch_kernel<decltype(v)::value>; });
}
// ---- ground reflection (kernels.h): as the ground pass, the HBM variant keeps the block's area in dynamic LDS --------------
hipError_t launch_reflection(const ReflectionFrame& f, const ReflectionShape& shape, int view, hipStream_t stream) {
    if (shape.max_bounces > kReflectMaxBounces) return hipErrorInvalidValue;  // the per-lane stack
    const size_t dyn = reflection_lds_bytes(f, shape);
    return launch_tile_pass(f, 1, shape, shape.tiles, view, dyn, dyn, stream, [](auto v) { return reflection_kernel<decltype(v)::value>; });
}
hipError_t launch_reflection_batch(const ReflectionFrame* d_table, int n_frames, const ReflectionShape& shape, int view, size_t max_dyn, hipStream_t stream) {
    if (shape.max_bounces > kReflectMaxBounces) return hipErrorInvalidValue;
    return launch_tile_pass(ReflectionTable(d_table), n_frames, shape, shape.tiles, view, max_dyn, max_dyn, stream,
                            [](auto v) { return reflection_batch_kernel<decltype(v)::value>; });
}
// ---- light layers (kernels.h): `shade` when visibility or direct is asked for, `occlusion` when that plane is; the HBM variants
// keep the block's area in dynamic LDS
hipError_t launch_light(const ShadeFrame& f, const ShadeShape& shape, int view, hipStream_t stream) {
    hipError_t e = hipSuccess;
    if (f.visibility || f.direct) {
        const size_t dyn = shade_lds_bytes(f, shape);
        e = launch_tile_pass(f, 1, shape, shape.tiles, view, dyn, dyn, stream, [](auto v) { return shade_kernel<decltype(v)::value>; });
    }
    if (e == hipSuccess && f.occlusion) {
        const size_t dyn = occlusion_lds_bytes(f);
        e = launch_tile_pass(f, 1, shape, shape.tiles, view, dyn, dyn, stream, [](auto v) { return occlusion_kernel<decltype(v)::value>; });
    }
    return e;
}
hipError_t launch_light_batch(const ShadeFrame* d_table, int n_frames, const ShadeShape& shape, int view, bool shade, size_t shade_dyn, bool occlusion,
                              size_t occlusion_dyn, hipStream_t stream) {
    hipError_t e = hipSuccess;
    if (shade)
        e = launch_tile_pass(ShadeTable(d_table), n_frames, shape, shape.tiles, view, shade_dyn, shade_dyn, stream,
                             [](auto v) { return shade_batch_kernel<decltype(v)::value>; });
    if (e == hipSuccess && occlusion)
        e = launch_tile_pass(ShadeTable(d_table), n_frames, shape, shape.tiles, view, occlusion_dyn, occlusion_dyn, stream,
                             [](auto v) { return occlusion_batch_kernel<decltype(v)::value>; });
    return e;
}
// ---- light bake (kernels.h): a workgroup per 256 pool texels of the largest frame; `bake_shade` when visibility or direct is asked
// for — or no occlusion plane, then for position / normal alone —, `bake_occlusion` when that plane is; position and normal by the
// first kernel that runs
template <class Arg, class KernelOf>
static hipError_t launch_bake_pass(const Arg& arg, int n_frames, const BakeShape& shape, int view, size_t dyn, hipStream_t stream, KernelOf kernel_of) {
    if (shape.max_units <= 0 || n_frames <= 0) return hipSuccess;
    if (n_frames > kLayersBatchMaxFrames || shape.grid < 1 || shape.grid > kBakeMaxGrid) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>(shape.max_units < kLayersGrid ? shape.max_units : kLayersGrid), static_cast<unsigned>(n_frames));
    with_view(view, [&](auto v) { hipLaunchKernelGGL(kernel_of(v), grid, dim3(kBlock), dyn, stream, arg, shape); });
    return hipGetLastError();
}
hipError_t launch_bake(const BakeFrame& f, const BakeShape& shape, int view, hipStream_t stream) {
    hipError_t e = hipSuccess;
    BakeShape sh = shape;
    const bool shade = f.visibility || f.direct || !f.occlusion;
    if (shade) {
        sh.geometry = 1, sh.rays = (f.visibility || f.direct) ? 1 : 0;
        e = launch_bake_pass(f, 1, sh, view, bake_shade_lds_bytes(f, sh), stream, [](auto v) { return bake_shade_kernel<decltype(v)::value>; });
    }
    if (e == hipSuccess && f.occlusion) {
        sh.geometry = shade ? 0 : 1, sh.rays = 1;
        e = launch_bake_pass(f, 1, sh, view, bake_occlusion_lds_bytes(f), stream, [](auto v) { return bake_occlusion_kernel<decltype(v)::value>; });
    }
    return e;
}
hipError_t launch_bake_batch(const BakeFrame* d_table, int n_frames, const BakeShape& shape, int view, bool shade, size_t shade_dyn, bool occlusion,
                             size_t occlusion_dyn, hipStream_t stream) {
    hipError_t e = hipSuccess;
    BakeShape sh = shape;
    const bool first = shade || !occlusion;
    if (first) {
        sh.geometry = 1, sh.rays = shade ? 1 : 0;
        e = launch_bake_pass(BakeTable(d_table), n_frames, sh, view, shade_dyn, stream, [](auto v) { return bake_shade_batch_kernel<decltype(v)::value>; });
    }
    if (e == hipSuccess && occlusion) {
        sh.geometry = first ? 0 : 1, sh.rays = 1;
        e = launch_bake_pass(BakeTable(d_table), n_frames, sh, view, occlusion_dyn, stream, [](auto v) { return bake_occlusion_batch_kernel<decltype(v)::value>; });
    }
    return e;
}
// ---- light layers and bake under extra lights (kernels.h): `shade_lights` / `bake_shade_lights` alone, with the single-light
// kernels' LDS (the area does not grow with the lights); the occlusion plane goes through launch_light / launch_bake
hipError_t launch_light_multi(const ShadeLightsFrame& f, const ShadeShape& shape, int view, hipStream_t stream) {
    const size_t dyn = shade_lds_bytes(f, shape);
    return launch_tile_pass(f, 1, shape, shape.tiles, view, dyn, dyn, stream, [](auto v) { return shade_lights_kernel<decltype(v)::value>; });
}
hipError_t launch_light_multi_batch(const ShadeLightsFrame* d_table, int n_frames, const ShadeShape& shape, int view, size_t max_dyn, hipStream_t stream) {
    return launch_tile_pass(ShadeLightsTable(d_table), n_frames, shape, shape.tiles, view, max_dyn, max_dyn, stream,
                            [](auto v) { return shade_lights_batch_kernel<decltype(v)::value>; });
}
hipError_t launch_bake_multi(const BakeLightsFrame& f, const BakeShape& shape, int view, hipStream_t stream) {
    BakeShape sh = shape;
    sh.geometry = 1, sh.rays = 1;
    return launch_bake_pass(f, 1, sh, view, bake_shade_lds_bytes(f, sh), stream, [](auto v) { return bake_shade_lights_kernel<decltype(v)::value>; });
}
hipError_t launch_bake_multi_batch(const BakeLightsFrame* d_table, int n_frames, const BakeShape& shape, int view, size_t max_dyn, hipStream_t stream) {
    BakeShape sh = shape;
    sh.geometry = 1, sh.rays = 1;
    return launch_bake_pass(BakeLightsTable(d_table), n_frames, sh, view, max_dyn, stream, [](auto v) { return bake_shade_lights_batch_kernel<decltype(v)::value>; });
}
hipError_t launch_pick(const uint8_t* scene, const LayersShape& shape, const int32_t* d_xy, int n, mcrt_surface* d_out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(pick_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, scene, shape, d_xy, n, d_out);
    return hipGetLastError();
}
// ---- studio shot (kernels.h): a workgroup per 256 pixels, at most kLayersGrid per frame (the kernel strides) ----------------
static unsigned shot_grid(const ShotShape& sh) {
    const long long px = static_cast<long long>(sh.cfg.width) * sh.cfg.height;
    const long long groups = (px + kBlock - 1) / kBlock;
    return static_cast<unsigned>(groups < kLayersGrid ? groups : kLayersGrid);
}
// With bounds every workgroup that sees content ends on the frame's entry, and the atomics of one entry queue up.  So a launch
// with bounds takes no more workgroups than the chip holds at once (256 CUs x 8 of these workgroups), shared among its frames:
// fewer, longer workgroups — the lanes take more trips — and as many atomics fewer.
constexpr unsigned kBoundsGroups = 2048;
static unsigned shot_bounds_grid(const ShotShape& sh, const int32_t* d_bounds, int n_frames) {
    const unsigned groups = shot_grid(sh);
    if (!d_bounds) return groups;
    const unsigned share = kBoundsGroups / static_cast<unsigned>(n_frames);
    return share < 1u ? 1u : share < groups ? share : groups;
}
static bool shot_shape_ok(const ShotShape& sh, const int32_t* d_bounds) {  // bounds come with the cut-out alone
    return sh.cfg.width > 0 && sh.cfg.height > 0 && static_cast<long long>(sh.cfg.width) * sh.cfg.height < (1ll << 31) && sh.page >= MCRT_PAGE_COLOR &&
           sh.page <= MCRT_PAGE_TRANSPARENT && (!d_bounds || sh.page == MCRT_PAGE_TRANSPARENT);
}
hipError_t launch_shot(const ShotFrame& f, const ShotShape& shape, int32_t* d_bounds, hipStream_t stream) {
    if (!shot_shape_ok(shape, d_bounds) || !f.figure || (!f.out && !f.out8)) return hipErrorInvalidValue;
    if (shape.page == MCRT_PAGE_TRANSPARENT)
        hipLaunchKernelGGL(shot_kernel<true>, dim3(shot_bounds_grid(shape, d_bounds, 1)), dim3(kBlock), 0, stream, f, shape, d_bounds);
    else
        hipLaunchKernelGGL(shot_kernel<false>, dim3(shot_grid(shape)), dim3(kBlock), 0, stream, f, shape, d_bounds);
    return hipGetLastError();
}
hipError_t launch_shot_batch(const ShotFrame* d_table, int n_frames, const ShotShape& shape, int32_t* d_bounds, hipStream_t stream) {
    if (n_frames <= 0) return hipSuccess;
    if (!shot_shape_ok(shape, d_bounds) || n_frames > kLayersBatchMaxFrames) return hipErrorInvalidValue;
    const dim3 grid(shot_bounds_grid(shape, d_bounds, n_frames), static_cast<unsigned>(n_frames));
    if (shape.page == MCRT_PAGE_TRANSPARENT)
        hipLaunchKernelGGL(shot_batch_kernel<true>, grid, dim3(kBlock), 0, stream, ShotTable(d_table), shape, d_bounds);
    else
        hipLaunchKernelGGL(shot_batch_kernel<false>, grid, dim3(kBlock), 0, stream, ShotTable(d_table), shape, d_bounds);
    return hipGetLastError();
}
hipError_t launch_shot_bounds_init(int32_t* d_bounds, int n, int width, int height, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (!d_bounds) return hipErrorInvalidValue;
    const long long words = 4ll * n;
    hipLaunchKernelGGL(shot_bounds_init_kernel, dim3(static_cast<unsigned>((words + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, d_bounds, n, width, height);
    return hipGetLastError();
}
// ---- skins on resident scenes (kernels.h) -----------------------------------------------------------
static bool skin_shape_ok(const SkinPaintShape& sh) {  // what the kernel's fixed LDS image and its 4-bit mesh field hold
    return sh.tables && sh.n_texels > 0 && sh.n_texels <= kSkinMaxTexels && sh.n_meshes > 0 && sh.n_meshes <= kSkinMaxMeshes &&
           (sh.skin_bytes == 64 * 64 * 4 || sh.skin_bytes == 64 * 32 * 4) && sh.alpha_words == static_cast<uint32_t>((sh.n_texels + 15) / 16);
}
hipError_t launch_skin_paint(const SkinPaintFrame& f, const SkinPaintShape& shape, hipStream_t stream) {
    if (!skin_shape_ok(shape) || !f.scene || !f.skin) return hipErrorInvalidValue;
    hipLaunchKernelGGL(skin_paint_kernel, dim3(1), dim3(kSkinBlock), 0, stream, f, shape);
    return hipGetLastError();
}
hipError_t launch_skin_paint_batch(const SkinPaintFrame* d_table, int n_frames, const SkinPaintShape shapes[kSkinBatchShapes], hipStream_t stream) {
    if (n_frames <= 0) return hipSuccess;
    // both shapes are checked whatever the frames name: a workgroup may take either, and one image size fills the LDS image
    if (!skin_shape_ok(shapes[0]) || !skin_shape_ok(shapes[1]) || shapes[0].skin_bytes != shapes[1].skin_bytes || n_frames > kLayersBatchMaxFrames)
        return hipErrorInvalidValue;
    const dim3 grid(1, static_cast<unsigned>(n_frames));
    const SkinPaintShape &a = shapes[0], &b = shapes[1];
    const bool one_kind = a.tables == b.tables && a.n_texels == b.n_texels && a.n_meshes == b.n_meshes && a.mesh_offset == b.mesh_offset &&
                          a.texel_offset == b.texel_offset && a.alpha_offset == b.alpha_offset && a.alpha_words == b.alpha_words;
    if (one_kind)  // the single-shape kernel, whatever the frames name
        hipLaunchKernelGGL(skin_paint_batch_kernel, grid, dim3(kSkinBlock), 0, stream, SkinPaintTable(d_table), shapes[0]);
    else
        hipLaunchKernelGGL(skin_paint_mixed_kernel, grid, dim3(kSkinBlock), 0, stream, SkinPaintTable(d_table), shapes[0], shapes[1]);
    return hipGetLastError();
}
// ---- capes on resident scenes (kernels.h) -----------------------------------------------------------
// 16-byte texel stores, 4-byte words; the parts in the blob's order.  (The frames of a batch are in device memory: their
// caller, set_capes_batch_device, checks each with this before it uploads them.)
bool cape_frame_ok(const CapePaintFrame& f) {
    return f.scene && (reinterpret_cast<uintptr_t>(f.cape) & 3u) == 0 && f.flags_offset % 4u == 0 && f.texel_offset % 16u == 0 && f.alpha_offset % 4u == 0 &&
           f.flags_offset + 4u <= f.texel_offset && f.texel_offset + static_cast<uint32_t>(kCapeTexels) * 16u <= f.alpha_offset;
}
hipError_t launch_cape_paint(const CapePaintFrame& f, const CapePaintShape& shape, hipStream_t stream) {
    if (!shape.tables || !cape_frame_ok(f)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cape_paint_kernel, dim3(1), dim3(kCapeBlock), 0, stream, f, shape);
    return hipGetLastError();
}
hipError_t launch_cape_paint_batch(const CapePaintFrame* d_table, int n_frames, const CapePaintShape& shape, hipStream_t stream) {
    if (n_frames <= 0) return hipSuccess;
    if (!shape.tables || n_frames > kLayersBatchMaxFrames) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cape_paint_batch_kernel, dim3(1, static_cast<unsigned>(n_frames)), dim3(kCapeBlock), 0, stream, CapePaintTable(d_table), shape);
    return hipGetLastError();
}
// ---- views of resident scenes (kernels.h) -------------------------------------------------------------
static bool view_shape_ok(const SceneViewShape& sh) {  // three chunks per lane; the mesh table inside the prefix
    return sh.n_chunks > 0 && sh.n_chunks <= kViewMaxChunks && sh.mesh_offset % 16u == 0 && sh.n_meshes >= 0 && sh.n_meshes <= kCapedMaxMeshes &&
           sh.mesh_offset / 16u + kMeshChunks * static_cast<uint32_t>(sh.n_meshes) <= static_cast<uint32_t>(sh.n_chunks);
}
hipError_t launch_scene_view(const SceneViewFrame& f, const SceneViewShape& shape, hipStream_t stream) {
    if (!view_shape_ok(shape) || !f.scene || !f.table || (reinterpret_cast<uintptr_t>(f.table) & 15u) != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scene_view_kernel, dim3(1), dim3(kViewBlock), 0, stream, f, shape);
    return hipGetLastError();
}
hipError_t launch_scene_view_batch(const SceneViewFrame* d_table, int n_frames, const SceneViewShape& shape, hipStream_t stream) {
    if (n_frames <= 0) return hipSuccess;
    if (!view_shape_ok(shape) || n_frames > kLayersBatchMaxFrames) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scene_view_batch_kernel, dim3(1, static_cast<unsigned>(n_frames)), dim3(kViewBlock), 0, stream, SceneViewTable(d_table), shape);
    return hipGetLastError();
}

}  // namespace mcrt
