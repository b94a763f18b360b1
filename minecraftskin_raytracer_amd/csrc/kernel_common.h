// kernel_common.h — device-side helpers that more than one kernel file uses (render_kernels.hip, pass_kernels.hip,
// util_kernels.hip): tile geometry, the scene tables staged in LDS and the kernel variants built on them, the block-wide
// rank, the light's disk samples, the RGBA8 quantisation, the launch-side dispatch over the variants, and the phases the
// stand-alone passes share (the (item, sample) ray loop, the shadow-bundle resolver, the AO stream).
#ifndef MCRT_KERNEL_COMMON_H
#define MCRT_KERNEL_COMMON_H

#include "kernels.h"
#include "rt_core.h"

#include <type_traits>

// Verification hooks.  tools/decide_check.sh builds a variant of the library with -DMCRT_KERNEL_HOOKS='"decide_check_hooks.h"'
// (tools/decide_check_hooks.h: every record `lit` decides is traced as well and contradictions are counted and printed);
// the product build compiles the hooks to nothing.  tools/gpu_ground.py builds another variant with tools/ground_class_hooks.h
// (the ground pass's hook: pass_kernels.hip), tools/gpu_ground_occlusion.py one with tools/ground_occlusion_class_hooks.h.
#ifdef MCRT_KERNEL_HOOKS
#include MCRT_KERNEL_HOOKS
#else
#define MCRT_HOOK_LIT_SHARED
#define MCRT_HOOK_LIT_CLASSIFIED(known, undecided, cand, O)
#define MCRT_HOOK_LIT_SHADED(lit, r)
#define MCRT_HOOK_RESOLVE_BEGIN()
#endif

namespace mcrt {

using namespace rt;

// n / d for a divisor that is the same for the whole wave: a shift when it is a power of two (tile widths of 32,
// 4 samples per pixel: the usual case) instead of the ~25-instruction expansion of a 32-bit division.
struct UDiv {
    unsigned d;
    int shift;  // log2(d), or -1
    __device__ __forceinline__ explicit UDiv(unsigned dv) : d(dv), shift((dv & (dv - 1u)) == 0u && dv != 0u ? static_cast<int>(__builtin_ctz(dv)) : -1) {}
    __device__ __forceinline__ unsigned div(unsigned n) const { return shift >= 0 ? n >> shift : n / d; }
};

// ---------------------------------------------------------------------------------------------
// Parameters by phase.  A kernel of the render pipeline holds its RenderParams where scalar loads reach them at any time:
// in its own kernarg segment (the single-frame entries take them by value, as their FIRST argument) or in the batch's
// device-resident table — constant address space either way.  Read through a plain reference, the compiler loads every
// field a kernel will ever need at its entry and keeps it live across the persistent item loop: 106 SGPRs do not hold
// ~150 dwords of parameters and 25 workspace pointers beside the loop's own state, and the overflow is parked in VGPR
// lanes (v_writelane / v_readlane: VALU work inside the hot loops, DESIGN.md §4 "Scalar registers").  So the item loops
// take the parameters BY PHASE: phase_params(pp) at a phase's start gives a reference the optimiser cannot merge with an
// earlier one — the pointer passes through an empty asm in a scalar register pair — and what the phase reads comes in
// by scalar loads right there (no VALU slot; other waves hide the wait) and dies with the phase.  Only the pointer
// itself (2 SGPRs) lives across the loops.
// ---------------------------------------------------------------------------------------------
using ParamPtr = const __attribute__((address_space(4))) RenderParams*;
__device__ __forceinline__ const RenderParams& phase_params(ParamPtr pp) {
    asm volatile("" : "+s"(pp));
    return *(const RenderParams*)pp;
}
// the by-value RenderParams that is a kernel's first argument, in its kernarg segment
__device__ __forceinline__ ParamPtr kernarg_params() { return (ParamPtr)__builtin_amdgcn_kernarg_segment_ptr(); }

// ---------------------------------------------------------------------------------------------
// tile geometry helpers (TileRenderer::generateTiles, tile_renderer.cpp:18-39)
// ---------------------------------------------------------------------------------------------
struct TileGeom {
    int x, y, w, h;
    int owned_row;  // index of this tile's row among the rows this launch owns
    int frame_tile;  // row-major index of the tile in the whole frame (its slot in a background or draw plate, kernels.h)
};

// ---------------------------------------------------------------------------------------------
// work units of a touched tile (WaveSpace::units): a pixel range of the tile's row-major order, or a block of the tile
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kUnitBlock = 1u << 31;  // in .x of a unit record: the record is a block
__device__ __forceinline__ int unit_tile(const uint4& ud) { return static_cast<int>(ud.x & ~kUnitBlock); }
__device__ __forceinline__ uint32_t unit_pixels(const uint4& ud) { return (ud.x & kUnitBlock) ? (ud.z & 0xffffu) * (ud.z >> 16) : ud.z - ud.y; }
// Pixel k (< unit_pixels) of unit ud, in the unit's own order — a range: the tile's row-major order; a block: the block's —
// as (lx, ly) in its tile tg.  The one place that knows the two forms: a sample's draws sit at ((ly * tg.w + lx) * spp + s) *
// draws_per_sample of the tile's stream whichever unit holds the pixel, and its slot is the unit's slot base + k * spp + s.
// Both forms are one: pixel k lies k + koff pixels into a rectangle that is `by_w.d` wide and starts at (x0, y0) of the tile —
// the block itself, or the whole tile with koff = the range's first pixel.  A kernel that walks a unit forms the map once.
struct UnitMap {
    uint32_t koff, x0, y0;
    UDiv by_w;
    __device__ __forceinline__ UnitMap(const uint4& ud, const TileGeom& tg)
        : koff((ud.x & kUnitBlock) ? 0u : ud.y), x0((ud.x & kUnitBlock) ? (ud.y & 0xffffu) : 0u), y0((ud.x & kUnitBlock) ? (ud.y >> 16) : 0u),
          by_w((ud.x & kUnitBlock) ? (ud.z & 0xffffu) : static_cast<uint32_t>(tg.w)) {}
    // column and row of pixel k in that rectangle: (lx, ly) = (x0 + col, y0 + row)
    __device__ __forceinline__ void rel(uint32_t k, uint32_t& col, uint32_t& row) const {
        const uint32_t q = k + koff;
        row = by_w.div(q);
        col = q - row * by_w.d;
    }
    __device__ __forceinline__ void pixel(uint32_t k, int& lx, int& ly) const {
        uint32_t col, row;
        rel(k, col, row);
        lx = static_cast<int>(x0 + col);
        ly = static_cast<int>(y0 + row);
    }
};
__device__ __forceinline__ void unit_pixel(const uint4& ud, const TileGeom& tg, uint32_t k, int& lx, int& ly) { UnitMap(ud, tg).pixel(k, lx, ly); }
// RGBA8 quantisation `(u8)(clamp(c,0,1)*255+0.5)` (image_writer.cpp:18-22 ≡ image.cpp:31-36)
__device__ __forceinline__ uchar4 quantize_pixel(float4 c) {
    uchar4 q;
    q.x = static_cast<unsigned char>(sclamp(c.x, 0.0f, 1.0f) * 255.0f + 0.5f);
    q.y = static_cast<unsigned char>(sclamp(c.y, 0.0f, 1.0f) * 255.0f + 0.5f);
    q.z = static_cast<unsigned char>(sclamp(c.z, 0.0f, 1.0f) * 255.0f + 0.5f);
    q.w = static_cast<unsigned char>(sclamp(c.w, 0.0f, 1.0f) * 255.0f + 0.5f);
    return q;
}

// ---------------------------------------------------------------------------------------------
// primary-ray culling mask of a tile
// ---------------------------------------------------------------------------------------------
// lens_pad: how far a thin-lens ray can displace the image of a point of this mesh, in the bound's
// units (0 for the pinhole camera)
__device__ __forceinline__ bool mesh_touches_tile(const FlatMesh& m, const TileGeom& t, const mcrt_config& cfg,
                                                  float aspect, float lens_pad) {
    float u0 = m.screen[0], v0 = m.screen[1], u1 = m.screen[2], v1 = m.screen[3];
    if (u0 > u1) return true;  // no bound available
    u0 -= lens_pad, v0 -= lens_pad, u1 += lens_pad, v1 += lens_pad;
    const float W = static_cast<float>(cfg.width), H = static_cast<float>(cfg.height);
    // tile extent padded by 2 pixels, in the bound's units (x: (2u-1)*aspect, y: 1-2v, +y up)
    float tu0 = (2.0f * (static_cast<float>(t.x) - 2.0f) / W - 1.0f) * aspect - 1e-3f * aspect - 1e-3f;
    float tu1 = (2.0f * (static_cast<float>(t.x + t.w) + 2.0f) / W - 1.0f) * aspect + 1e-3f * aspect + 1e-3f;
    float tv1 = 1.0f - 2.0f * (static_cast<float>(t.y) - 2.0f) / H + 2e-3f;
    float tv0 = 1.0f - 2.0f * (static_cast<float>(t.y + t.h) + 2.0f) / H - 2e-3f;
    return !(u1 < tu0 || u0 > tu1 || v1 < tv0 || v0 > tv1);
}

// ---------------------------------------------------------------------------------------------
// scene tables staged in LDS: what candidates index PER LANE (face → texture table, alpha bits)
// ---------------------------------------------------------------------------------------------
struct LdsTables {
    const MCRT_LDS uint32_t* abits;
    const MCRT_LDS int* faces;
    const MCRT_LDS float* mtab;
};
// dyn = dynamic LDS base; layout [face table: 4 ints per (mesh, face)][mesh table: kMeshTabWords per
// mesh][alpha words].  Collective.  The offsets below and scene_tables_lds_bytes (launch_shapes.h), by which every
// launch sizes this area, are one formula: s_abits starts at scene_tables_lds_bytes(lds_face_entries, 0) and ends at
// scene_tables_lds_bytes(lds_face_entries, lds_alpha_words) — change them together.
__device__ __forceinline__ LdsTables stage_tables(const SceneView& g, const int lds_face_entries, const int lds_alpha_words, unsigned char* dyn) {
    int* s_faces = reinterpret_cast<int*>(dyn);
    float* s_mtab = reinterpret_cast<float*>(dyn + static_cast<size_t>(lds_face_entries) * 16);
    const int n_meshes = lds_face_entries / 6;
    uint32_t* s_abits = reinterpret_cast<uint32_t*>(dyn + static_cast<size_t>(lds_face_entries) * 16 +
                                                    static_cast<size_t>(n_meshes) * kMeshTabWords * 4);
    for (int i = threadIdx.x; i < lds_alpha_words; i += blockDim.x) s_abits[i] = g.abits[i];
    for (int i = threadIdx.x; i < lds_face_entries; i += blockDim.x) {
        const FlatMesh& fm = g.meshes[i / 6];
        const int f = i - (i / 6) * 6;
        s_faces[4 * i + 0] = fm.tex_off[f];
        s_faces[4 * i + 1] = fm.tex_w[f];
        s_faces[4 * i + 2] = fm.tex_h[f];
        s_faces[4 * i + 3] = 0;
    }
    for (int i = threadIdx.x; i < n_meshes; i += blockDim.x) {
        const FlatMesh& fm = g.meshes[i];
        float* t = s_mtab + i * kMeshTabWords;
        t[0] = fm.lo[0], t[1] = fm.lo[1], t[2] = fm.lo[2];
        t[3] = fm.hi[0], t[4] = fm.hi[1], t[5] = fm.hi[2];
        t[6] = __uint_as_float(fm.flags);
        t[7] = 0.0f;
        t[8] = fm.pivot[0], t[9] = fm.pivot[1], t[10] = fm.pivot[2];
        t[11] = 0.0f;
        t[12] = fm.inv_z_cos, t[13] = fm.inv_z_sin, t[14] = fm.inv_x_cos, t[15] = fm.inv_x_sin;
        t[16] = fm.fwd_x_cos, t[17] = fm.fwd_x_sin, t[18] = fm.fwd_z_cos, t[19] = fm.fwd_z_sin;
        t[20] = fm.sphere[0], t[21] = fm.sphere[1], t[22] = fm.sphere[2], t[23] = fm.sphere[3];
    }
    __syncthreads();
    return LdsTables{(const MCRT_LDS uint32_t*)s_abits, (const MCRT_LDS int*)s_faces, (const MCRT_LDS float*)s_mtab};
}
__device__ __forceinline__ LdsTables stage_tables(const SceneView& g, const RenderParams& p, unsigned char* dyn) {
    return stage_tables(g, p.lds_face_entries, p.lds_alpha_words, dyn);
}
template <int kView>
struct ViewSel {
    using type = SceneViewLdsT<kView == kViewLds>;
    static __device__ __forceinline__ type make(const SceneView& g, const RenderParams& p, unsigned char* dyn) {
        LdsTables t = stage_tables(g, p, dyn);
        return view_with_lds<kView == kViewLds>(g, t.abits, t.faces, t.mtab);
    }
};
template <>
struct ViewSel<kViewHbm> {
    using type = SceneView;
    static __device__ __forceinline__ type make(const SceneView& g, const RenderParams&, unsigned char*) { return g; }
};
// The view of variant kView, made the first time a unit of the workgroup needs it: the passes stage the scene tables at
// their first touched tile only (a bake, which has no tiles, at once).  Collective for the LDS variants (stage_tables):
// all 256 threads reach it under uniform control flow, and `needed` and `staged` are the same in every thread.
template <int kView>
__device__ __forceinline__ void stage_view_once(const SceneView& g, const int lds_face_entries, const int lds_alpha_words, unsigned char* dyn, const bool needed,
                                                typename ViewSel<kView>::type& sc, bool& staged) {
    if (needed && !staged) {
        if constexpr (kView == kViewHbm) {
            sc = g;
        } else {
            const LdsTables t = stage_tables(g, lds_face_entries, lds_alpha_words, dyn);
            sc = view_with_lds<kView == kViewLds>(g, t.abits, t.faces, t.mtab);
        }
        staged = true;
    }
}
// launch side: calls f(std::integral_constant<int, kView>{}) for the variant `view` names, so a launcher writes its
// kernel template once: [&](auto v) { ... kernel<decltype(v)::value> ... }
template <class F>
static void with_view(int view, F&& f) {
    if (view == kViewLdsUnposed) return f(std::integral_constant<int, kViewLdsUnposed>{});
    if (view == kViewLds) return f(std::integral_constant<int, kViewLds>{});
    return f(std::integral_constant<int, kViewHbm>{});
}

// Rank of this thread's item among the workgroup's flagged items, and their total: ballot per wave,
// four wave counts through LDS.  COLLECTIVE (two barriers: the counts are reusable right after): all 256 threads must
// reach it under uniform control flow — a barrier under a divergent branch hangs the device.
__device__ __forceinline__ int block_rank(bool flag, int* s_wcnt, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(flag);
    if (lane == 0) s_wcnt[wave] = __popcll(bal);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int wv = 0; wv < kBlock / 64; ++wv) {
        const int c = s_wcnt[wv];
        if (wv < wave) before += c;
        total += c;
    }
    __syncthreads();
    return before + __popcll(bal & ((1ull << lane) - 1ull));
}

// One element of a sample-table row (kernels.h): what light_sample_on_frame makes of the draws d0, d1 before the light enters.
__device__ __forceinline__ float4 sample_row_element(const float d0, const float d1) {
    float sn, cs;
    mcrt_sincosf(kTwoPi * d0, &sn, &cs);
    return make_float4(cs, sn, sqrt_pos(d1), 0.0f);
}
// The S disk sample positions of the point P whose shadow seed is `seed`, from the seed's row of the device's sample table:
// light_sample_on_frame's expressions on the row's {cs, sn, sq}.  False, and nothing written, where the table does not
// serve: no table, more samples than a row holds, a seed outside the window.
__device__ __forceinline__ bool sample_row_positions(const SceneView& scg, const float4* __restrict__ sample_table, const uint32_t seed, const V3 P, const int S,
                                                     float* __restrict__ dst) {
    const uint32_t row = seed + kSampleWindowHalf;  // wraps: the window is centred on seed 0
    if (!sample_table || S > kSampleRow || row >= kSampleWindow) return false;
    const float4* __restrict__ src = sample_table + static_cast<size_t>(row) * kSampleRow;
    float4 e[kSampleRow];
#pragma unroll
    for (int i = 0; i < kSampleRow; ++i) e[i] = src[i];  // the whole line, whatever S is: the loads leave together
    const LightFrame frame = light_frame(scg, P);
    const float radius = scg.hdr->light_radius;
    const V3 lpos = ld3(scg.hdr->light_pos);
#pragma unroll
    for (int i = 0; i < kSampleRow; ++i) {
        if (i < S) {
            const float rr = radius * e[i].z;
            const V3 off = frame.tangent * (rr * e[i].x) + frame.bitangent * (rr * e[i].y);
            const V3 t = lpos + off;
            dst[3 * i + 0] = t.x;
            dst[3 * i + 1] = t.y;
            dst[3 * i + 2] = t.z;
        }
    }
    return true;
}

// The S disk sample positions of one shaded point (shading.cpp:35-53), by the lane that owns it (`lit`, the ground pass): from
// the seed's row of the device's sample table where that serves (sample_row_positions); else the truncated engine seeded for
// (P, depth) — mt[397] from the device's tables where they hold the seed, else the 397-step recurrence — and the light's
// frame at P.  dst: 3 * S floats.
__device__ __forceinline__ void disk_sample_positions(const SceneView& scg, const float4* __restrict__ sample_table, const uint32_t* __restrict__ seed_table,
                                                      const uint32_t* __restrict__ seed_table_full, const V3 P, const int depth, const int S,
                                                      float* __restrict__ dst) {
    MtShort rng;
    const uint32_t seed = shadow_seed(P, depth);
    if (sample_row_positions(scg, sample_table, seed, P, S, dst)) return;
    const uint32_t slot = seed + kSeedWindowHalf;  // wraps: the window is centred on seed 0
    if (seed_table && slot < kSeedWindow)
        rng.seed_known(seed, seed_table[slot]);  // mt[397] of this seed, from the device's table
    else if (seed_table_full)
        rng.seed_known(seed, seed_table_full[seed]);  // (a scene at another scale: its seeds leave the window)
    else
        rng.seed(seed);  // the 397-step recurrence
    const LightFrame frame = light_frame(scg, P);
    for (int i = 0; i < S; ++i) {
        const float d0 = rng.uniform();
        const float d1 = rng.uniform();
        const V3 t = light_sample_on_frame(scg, frame, d0, d1);
        dst[3 * i + 0] = t.x;
        dst[3 * i + 1] = t.y;
        dst[3 * i + 2] = t.z;
    }
}

// disk_sample_positions as the shadow resolver calls it — no sample table, no table of all seeds — for any light l (rt_core.h).
// Every light's call seeds from the same (P, depth): all lights see the same draws.  (A core of its own beside the form above:
// every shape that shared the two moved `lit`'s schedule — profiles/fold_twins/README.md.)
template <class Light>
__device__ __forceinline__ void disk_sample_positions_at(const Light& l, const uint32_t* __restrict__ seed_table, const V3 P, const int depth, const int S,
                                                         float* __restrict__ dst) {
    MtShort rng;
    const uint32_t seed = shadow_seed(P, depth);
    const uint32_t slot = seed + kSeedWindowHalf;  // wraps: the window is centred on seed 0
    if (seed_table && slot < kSeedWindow)
        rng.seed_known(seed, seed_table[slot]);  // mt[397] of this seed, from the device's table
    else
        rng.seed(seed);  // the 397-step recurrence
    const LightFrame frame = light_frame_at(l.position(), P);
    for (int i = 0; i < S; ++i) {
        const float d0 = rng.uniform();
        const float d1 = rng.uniform();
        const V3 t = light_sample_at(l, frame, d0, d1);
        dst[3 * i + 0] = t.x;
        dst[3 * i + 1] = t.y;
        dst[3 * i + 2] = t.z;
    }
}

// ---------------------------------------------------------------------------------------------
// phases the stand-alone passes share (pass_kernels.hip; DESIGN.md, "phases the passes share")
// ---------------------------------------------------------------------------------------------
// A lane per (item, sample): ray q = i * per + s belongs to item items[i], i < n_items, and counts[item] becomes the number
// of the item's `per` rays for which test(item, q) holds.  By ballot where a wave holds whole groups (per a power of two up
// to 64; per == 64 is the whole ballot, which a shift by 64 would not give), the first lane of a group storing its popcount;
// else by atomicAdd onto counts the caller has zeroed.  No barrier, but a ballot: all lanes of a wave reach it together
// (every lane of a wave runs the same number of turns).
template <class Test>
__device__ __forceinline__ void count_item_rays(const uint32_t* __restrict__ items, const uint32_t n_items, const uint32_t per, uint32_t* __restrict__ counts,
                                                Test test) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const bool pow2 = (per & (per - 1u)) == 0u && per <= 64u;
    const uint32_t n_rays = n_items * per;
    for (uint32_t q0 = tid & ~63u; q0 < n_rays; q0 += kBlock) {
        const uint32_t q = q0 + lane;
        bool flag = false;
        uint32_t k = 0;
        if (q < n_rays) {
            k = items[q / per];
            flag = test(k, q);
        }
        if (pow2) {
            const unsigned long long bal = __ballot(flag);
            if (q < n_rays && (lane & (per - 1u)) == 0u) {
                const unsigned long long grp = (per == 64u) ? bal : ((bal >> lane) & ((1ull << per) - 1ull));
                counts[k] = static_cast<uint32_t>(__popcll(grp));
            }
        } else if (flag) {
            atomicAdd(&counts[k], 1u);
        }
    }
}

// What the shadow resolver reads of a pass: the light and the shape's sampling, and the pass's LDS area — a candidate mask,
// an inside mask, a lit count and a list entry per lane, the sample positions of one pass of items (pass x S x 3 floats)
// and the four wave counts of block_rank.
struct ShadowBundles {
    V3 lpos;
    float R;          // the light's disk radius, 0 in the hard modes
    bool soft;        // S rays per item towards disk samples; otherwise one towards the light's centre (shading.cpp:31)
    int S;
    uint32_t pairs;   // rays per item
    uint32_t pass;    // items per pass
    bool decisions, inside_fast;
    const uint32_t* seed_table;
    unsigned long long* cand;
    unsigned long long* ins;
    uint32_t* lit;
    uint32_t* und;
    float* pos;
    int* wcnt;
};
template <class Light>
__device__ __forceinline__ ShadowBundles shadow_bundles(const Light& l, const int samples, const int pass, const int decisions, const int inside_fast,
                                                        const uint32_t* seed_table, unsigned long long* cand, unsigned long long* ins, uint32_t* lit,
                                                        uint32_t* und, float* pos, int* wcnt) {
    const float lradius = l.disk_radius();
    const bool soft = samples > 1 && !(lradius < 1e-4f);
    return ShadowBundles{l.position(), soft ? lradius : 0.0f, soft, samples, soft ? static_cast<uint32_t>(samples) : 1u, static_cast<uint32_t>(pass),
                         decisions != 0, inside_fast != 0, seed_table, cand, ins, lit, und, pos, wcnt};
}
// the visibility term of an item from its lit count: lit / S of computeSoftShadow, or the one ray of the hard modes
__device__ __forceinline__ float bundle_visibility(const ShadowBundles& b, const uint32_t lit) {
    return b.soft ? static_cast<float>(lit) / static_cast<float>(b.S) : (lit ? 1.0f : 0.0f);
}
// The lit counts of the workgroup's items towards light l, of which b was made (shadow_bundles(l, ...)): the scene's
// header_light, or a LightAt.  One per lane (item = lane index; `active`: the lane holds one, with shadow origin O):
// the whole-bundle decision (rt::bundle_classify, its candidates ANDed with tile_mask) and the inside masks by the item's
// lane; the undecided packed (block_rank); then in passes of b.pass items a lane per item forms the S disk sample positions
// of the engine seeded for (point, depth), and a lane per (item, sample) runs the exact any-hit test (count_item_rays).
// point_of(k, P, N): the point of item k and the normal its shadow rays leave along, read from the caller's LDS records.
// Returns whether the lane's item was undecided; `lit` takes its count (decided or traced) and stays as it is on a lane
// without an item.
// COLLECTIVE: two barriers of block_rank, then — only where the workgroup has undecided items — one before the passes, one
// per pass (and one between passes) and one behind the counts.  All 256 threads must reach it under uniform control flow;
// a barrier under a divergent branch hangs the device — a loop over lights around it has the same trip count in all of them.
// Behind it nothing of the area is read across lanes any more, so the next light's call may write it at once.
template <bool kPosed, class SV, class Light, class PointOf>
__device__ __forceinline__ bool resolve_shadow_bundles(const SceneView& scg, const SV& sc, const ShadowBundles b, const Light& l, const bool active,
                                                       const V3 O, const unsigned long long tile_mask, const int depth, PointOf point_of, uint32_t& lit) {
    const uint32_t tid = threadIdx.x;
    const V3 lpos = b.lpos;  // (a value of its own: selected against a load below, b.lpos would be selected by address and keep b in memory)
    bool undecided = false;
    // ---- a lane per item: the whole-bundle decision
    if (active) {
        unsigned long long cand;
        const int known = bundle_classify<kPosed>(scg, sc, O, lpos, b.R, static_cast<int>(b.pairs), b.decisions, cand);
        cand &= tile_mask;
        undecided = known < 0;
        b.cand[tid] = cand;
        b.ins[tid] = (undecided && b.inside_fast) ? origin_inside_boxes(sc, O, cand) : 0ull;
        if (!undecided) lit = static_cast<uint32_t>(known);
    }
    b.lit[tid] = 0u;
    int total = 0;
    const int rank = block_rank(undecided, b.wcnt, total);
    if (undecided) b.und[rank] = tid;
    const uint32_t n_und = static_cast<uint32_t>(total);
    if (n_und) __syncthreads();  // uniform
    for (uint32_t u0 = 0; u0 < n_und; u0 += b.pass) {  // uniform
        const uint32_t nu = min(b.pass, n_und - u0);
        if (u0) __syncthreads();  // the previous pass's rays have read the positions
        // ---- a lane per undecided item: its mt19937 stream and the S disk sample positions
        // (outside the seed table's window — points far out, at the horizon — the 397-step recurrence)
        if (b.soft && tid < nu) {
            V3 P, N;  // (N goes unused here: the accessor is inlined and its fetch of the normal falls away)
            point_of(b.und[u0 + tid], P, N);
            disk_sample_positions_at(l, b.seed_table, P, depth, b.S, b.pos + static_cast<size_t>(tid) * 3 * b.S);
        }
        __syncthreads();
        // ---- a lane per (undecided item, light sample)
        count_item_rays(b.und + u0, nu, b.pairs, b.lit, [&](const uint32_t k, const uint32_t q) __attribute__((always_inline)) {
            V3 P, N;
            point_of(k, P, N);
            const V3 target = b.soft ? ld3(b.pos + static_cast<size_t>(q) * 3) : lpos;
            return !in_shadow_masked(sc, P, N, target, b.cand[k], b.ins[k]);
        });
    }
    if (n_und) __syncthreads();  // the counts are complete
    if (undecided) lit = b.lit[tid];
    return undecided;
}

// The cosine-weighted directions of computeAO at P with unit normal N (raytracer.cpp:42-68), by the lane that owns the
// point: the truncated engine seeded for P — mt[397] from the device's table of all seeds where the handle holds it, one
// load instead of the 397-step recurrence — and the frame T, N, B; next() is the following world direction.
struct AoStream {
    V3 T, N, B;
    MtShort rng;
    __device__ __forceinline__ AoStream(const uint32_t* __restrict__ seed_table_full, const V3 P, const V3 Nu) : N(Nu) {
        T = (__builtin_fabsf(N.x) < 0.9f) ? normalize(cross(mk(1, 0, 0), N)) : normalize(cross(mk(0, 1, 0), N));
        B = cross(N, T);
        const uint32_t seed = ao_seed(P);
        if (seed_table_full)
            rng.seed_known(seed, seed_table_full[seed]);
        else
            rng.seed(seed);
    }
    __device__ __forceinline__ V3 next() {
        const float r1 = rng.uniform();
        const float r2 = rng.uniform();
        const float sinT = sqrt_pos(1.0f - r1);
        const float cosT = sqrt_pos(r1);
        float sn, cs;
        mcrt_sincosf(kTwoPi * r2, &sn, &cs);
        const V3 local = mk(sinT * cs, cosT, sinT * sn);
        return normalize(T * local.x + N * local.y + B * local.z);
    }
};

}  // namespace mcrt

#endif
