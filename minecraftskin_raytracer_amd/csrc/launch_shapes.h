// launch_shapes.h — the constants that the host planning (render_plan.cpp) shares with the kernels and their launchers
// (render_kernels.hip, pass_kernels.hip, kernel_common.h): block and grid sizes, LDS areas, the kernel variants, and the
// size of the scene tables a kernel stages in LDS.  Each is defined here alone.  Plain C++: no device construct.
#ifndef MCRT_LAUNCH_SHAPES_H
#define MCRT_LAUNCH_SHAPES_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rt {
constexpr int kMeshTabWords = 24;  // words per mesh of the mesh table staged in LDS (rt_core.h: SceneViewLdsT::mtab)
constexpr int kMtShortMax = 227;   // draws available from the two-recurrence form of mt19937 (rt_core.h: MtShort)
}  // namespace rt

namespace mcrt {

constexpr int kBlock = 256;
constexpr int kChunk = 256;        // work items per chunk: one per thread
#ifndef MCRT_PRIMARY_GRID
#define MCRT_PRIMARY_GRID 1280
#endif
constexpr int kPrimaryGrid = MCRT_PRIMARY_GRID; // persistent primary workgroups (5 per CU: the kernel is built for 5 waves per SIMD)
constexpr int kQueueGrid = 2048;   // workgroups of the queue kernels (grid-stride over device-side counts)
constexpr int kLitGridAlone = 4096;  // `lit` of a frame that has the device to itself
constexpr int kResolveGrid = 4096;
constexpr int kSharedGrid = 896;   // every kernel of a frame that shares the device (choose_grids): 3.5 workgroups per CU

constexpr int kStreamWaves = 4;  // `plan_tiles`: tiles per workgroup
constexpr int kSlabMinSpp = 33;  // `background_kernel` from this many samples per pixel on

// The flat pipeline keeps the records of every level at once: its arrays are laid out for up to
// kFlatMaxBounces reflection levels (1 + maxBounces records per sample slot in the worst case).
constexpr int kFlatMaxBounces = 8;
#ifndef MCRT_LIT_LDS_KB
#define MCRT_LIT_LDS_KB 25
#endif
constexpr size_t kLitLdsBytes = MCRT_LIT_LDS_KB * 1024;  // `lit`: LDS for the sample positions of the records whose rays are traced, per pass

// kernel variants by scene: kViewHbm — tables too large for LDS (reads HBM; any pose);
// kViewLds — tables in LDS, posed meshes present; kViewLdsUnposed — tables in LDS, no posed mesh
constexpr int kViewHbm = 0, kViewLds = 1, kViewLdsUnposed = 2;

// dynamic LDS of the scene tables a kernel stages (kernel_common.h: stage_tables, which lays them out in this order):
// face table (4 ints per (mesh, face)), mesh table (kMeshTabWords per mesh), alpha predicates
__host__ __device__ __forceinline__ size_t scene_tables_lds_bytes(int face_entries, int alpha_words) {
    return static_cast<size_t>(face_entries) * 16 + static_cast<size_t>(face_entries / 6) * rt::kMeshTabWords * 4 + static_cast<size_t>(alpha_words) * 4;
}

// where a pass's own area starts behind them: their size rounded up to 16 bytes — what the kernels carve by and the host sizes by
__host__ __device__ __forceinline__ size_t scene_tables_lds_span(int face_entries, int alpha_words) {
    return (scene_tables_lds_bytes(face_entries, alpha_words) + 15u) & ~static_cast<size_t>(15);
}

constexpr int kLayersGrid = 8192;  // layers and ground: workgroups per frame at most (the kernels stride over their units)

// The fixed LDS area of a pass, behind the tables: one struct per kernel body, an array of kBlock entries (one per lane) per
// member.  The body reaches its area through the struct and the host sizes it by sizeof (render_plan.cpp: *_lds_bytes), so
// the two cannot drift; the sample area of a pass (pass x samples x 3 floats) follows it.  The asserts pin today's sizes.
struct ShadowLanes {  // what the shadow resolver keeps per lane (kernel_common.h: ShadowBundles)
    unsigned long long cand[kBlock], ins[kBlock];  // candidate and inside masks
    uint32_t lit[kBlock], und[kBlock];             // lit counts, the undecided list
};
struct GroundArea {  // ground, ground occlusion
    unsigned long long cand[kBlock], ins[kBlock];  // candidate and inside masks
    float2 pxz[kBlock];                            // P.x, P.z
    uint32_t count[kBlock], list[kBlock];          // lit / occluded counts, the undecided / traced list
};
struct ReflectionArea {
    float4 rec[4 * kBlock];  // a hit record of four planes: point, normal, texel colour, ray
    ShadowLanes sh;
};
struct ShadeArea {
    float4 rec[3 * kBlock];  // a hit record of three planes: point, normal, texel colour
    ShadowLanes sh;
};
struct OcclusionArea {
    float4 rec[2 * kBlock];  // a hit record of two planes: point, normal
    unsigned long long mask[kBlock];  // the candidate mask
    uint32_t list[kBlock];            // the traced list
    float val[kBlock];                // the value
};
struct BakeShadeArea {
    float4 rec[2 * kBlock];  // a point record of two planes: point, normal
    float4 tex[kBlock];      // the texel record: colour,
    int4 own[kBlock];        // and owner face, texel, size
    ShadowLanes sh;
};
struct BakeOcclusionArea {
    float4 rec[2 * kBlock];  // the point record
    int4 own[kBlock];        // the owner-face half of the texel record
    unsigned long long mask[kBlock];
    uint32_t list[kBlock];
    float val[kBlock];
};
constexpr int kGroundPosBytes = 12 * 1024;  // ground: LDS for the sample positions of the undecided pixels of one pass
constexpr int kGroundFixedBytes = sizeof(GroundArea);
constexpr int kGroundOccDirBytes = 12 * 1024;  // ground occlusion: LDS for the A directions of the traced pixels of one pass
constexpr int kGroundOccFixedBytes = sizeof(GroundArea);
constexpr int kReflectPosBytes = 8 * 1024;  // reflection: LDS for the sample positions of the undecided level-1 hits of one pass
constexpr int kReflectFixedBytes = sizeof(ReflectionArea);
constexpr int kShadePosBytes = 8 * 1024;  // light layers, `shade`: LDS for the sample positions of the undecided hits of one pass
constexpr int kShadeFixedBytes = sizeof(ShadeArea);
constexpr int kOcclusionFixedBytes = sizeof(OcclusionArea);
constexpr int kBakePosBytes = 8 * 1024;  // light bake, `bake_shade`: LDS for the sample positions of the undecided points of one pass
constexpr int kBakeShadeFixedBytes = sizeof(BakeShadeArea);
constexpr int kBakeOcclusionFixedBytes = sizeof(BakeOcclusionArea);
static_assert(kGroundFixedBytes == kBlock * 32 && kReflectFixedBytes == kBlock * 88 && kShadeFixedBytes == kBlock * 72 && kOcclusionFixedBytes == kBlock * 48 &&
                  kBakeShadeFixedBytes == kBlock * 88 && kBakeOcclusionFixedBytes == kBlock * 64,
              "the passes' LDS areas: sizes the launches were tuned for, every member 16-byte aligned");

// Workgroups per frame of a batched launch.  Every kernel strides over its frame's device-side work, so the grid only
// shapes the schedule: a batch aims at kBatchTarget workgroups per launch (8 per CU of the 256 — twice what the largest
// stage keeps resident, enough to balance frames of unequal cost) spread evenly over its frames, never fewer than
// kBatchMinGrid per frame (a frame's share of the work never waits on a handful of workgroups) and never more than the
// frame would get on its own (choose_grids).  From 256 frames on the floor alone fills the target: kBatchMaxFrames.
constexpr int kBatchTarget = 2048;
constexpr int kBatchMinGrid = 8;

}  // namespace mcrt

#endif
