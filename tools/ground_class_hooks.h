// ground_class_hooks.h — measurement hook for csrc/pass_kernels.hip (NOT part of the product build).
// tools/gpu_ground.py builds a variant of the library with
//     -DMCRT_KERNEL_HOOKS='"ground_class_hooks.h"' -Itools
// in which the ground pass writes, instead of the visibility, how each pixel got it: 0 the ray misses the plane, 1 reached
// in a tile no mesh can shadow (culled by tile: no classification), 2 decided by rt::bundle_classify (lit by all samples or by
// none), 3 undecided: its rays were traced.  The tool counts the codes in the plane; the pass itself keeps no counters.
#ifndef MCRT_GROUND_CLASS_HOOKS_H
#define MCRT_GROUND_CLASS_HOOKS_H

#define MCRT_HOOK_LIT_SHARED
#define MCRT_HOOK_LIT_CLASSIFIED(known, undecided, cand, O)
#define MCRT_HOOK_LIT_SHADED(lit, r)
#define MCRT_HOOK_RESOLVE_BEGIN()
#define MCRT_HOOK_GROUND_PIXEL(vis, reached, culled, undecided) (vis) = !(reached) ? 0.0f : ((culled) ? 1.0f : ((undecided) ? 3.0f : 2.0f));

#endif
