// ground_occlusion_class_hooks.h — measurement hook for csrc/pass_kernels.hip (NOT part of the product build).
// tools/gpu_ground_occlusion.py builds a variant of the library with
//     -DMCRT_KERNEL_HOOKS='"ground_occlusion_class_hooks.h"' -Itools
// in which the ground-occlusion pass writes, instead of the occlusion, how each pixel got it: 0 the ray misses the plane, 1 reached
// in a tile no mesh can occlude (culled by tile: no plane point, no candidates), 2 reached without a candidate within the radius,
// 3 traced: its A rays were tested.  The tool counts the codes in the plane; the pass itself keeps no counters.
#ifndef MCRT_GROUND_OCCLUSION_CLASS_HOOKS_H
#define MCRT_GROUND_OCCLUSION_CLASS_HOOKS_H

#define MCRT_HOOK_LIT_SHARED
#define MCRT_HOOK_LIT_CLASSIFIED(known, undecided, cand, O)
#define MCRT_HOOK_LIT_SHADED(lit, r)
#define MCRT_HOOK_RESOLVE_BEGIN()
#define MCRT_HOOK_GROUND_OCCLUSION_PIXEL(occ, reached, culled, traced) (occ) = !(reached) ? 0.0f : ((culled) ? 1.0f : ((traced) ? 3.0f : 2.0f));

#endif
